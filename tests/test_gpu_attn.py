"""-m gpu: dense attention (csrc/attn.hip, nn._DenseAttnFn) and the Non-local decoder (models.decoder.dec_nonlocal).

The two entry points through the C ABI, element-wise against float64: references, operands, tables and the bounds
|got - ref64| <= EPS min(derived, CAL_MARGIN measured (1 + arg)) unit + floor are those of tests/attn_bounds.py;
tests/test_attn_cpu.py shows that these bounds on these inputs separate a float32 emulation of the kernels' order from the faulty
ones.  Inputs are read from pitched buffers whose gaps hold NaN; every output (and lse) lies in a sentinel frame that must
survive; the workspace is filled with NaN and followed by a sentinel tail; each call runs twice and must give the same bits.  The
backward call is handed the float64 forward's o and lse rounded to fp32 (attn_bounds: the references are evaluated on exactly
those values).

The decoder against its float64 twin (torch float64: F.conv2d, F.batch_norm, softmax(scale q k^T) v per head):
dec_nonlocal(in_planes=128, inner_planes=64, key_planes=32, value_planes=48, rep_head=True), the zero-initialised norm weight
moved away from 0, Dropout2d p = 0, 4 x 128 x 9 x 9, train mode, kv_stride 1 and 2, heads 1 and 2; figures and yardstick are those of
decoder_harness.assert_no_worse_than_deeplabv3: max|got - ref| / max|ref| of every output, dx and every
parameter gradient <= 2x the largest figure of dec_deeplabv3(in_planes=128, dilations=(1, 2, 12)) against its own twin.

The whole path: ResNet-50 + dec_nonlocal through ModelBuilder at 65 x 65 (a 9 x 9 decoder input)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import attn_bounds as B
from decoder_harness import (DEV, SENT, D, Rows, Ws, _merge, _ptr, _seq64, _show, _twice, assert_default_config_is_untouched,
                             assert_eval_forward_ignores_the_graph, assert_no_worse_than_deeplabv3, assert_replay_equals_eager,
                             build_net, call, decoder_cfg, net_input, query, step_calls, train_steps)
from split_bounds import recorded_calls

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
AF, AB = "u2pl_attn_fwd_f32", "u2pl_attn_bwd_f32"
ALL = ("dq", "dk", "dv")
SUBSETS = [tuple(n for i, n in enumerate(ALL) if m >> i & 1) for m in range(1, 8)]


def raw_fwd(q, k, v, heads, scale, pitched):
    """u2pl_attn_fwd_f32 -> (o [N, Pq, heads*Dv], lse [N, heads, Pq])"""
    N, Pq, HD = q.shape
    Pk, HDv = k.shape[1], v.shape[2]
    qin, kin, vin = (Rows(t.shape, pitched, np.nan, t) for t in (q, k, v))
    assert query("u2pl_attn_fwd_ws_floats", N, heads, Pq, Pk, HD // heads, HDv // heads) == 0

    def run(o):
        ws = Ws(0)
        call(AF, qin.ptr, qin.ld, kin.ptr, kin.ld, vin.ptr, vin.ld, scale, N, heads, Pq, Pk, HD // heads, HDv // heads, *_ptr(o["o"]),
             o["lse"].ptr, ws.buf)
        return ws
    r = _twice("attention forward", run, lambda: dict(o=Rows((N, Pq, HDv), pitched, SENT), lse=Rows((1, 1, N * heads * Pq), False, SENT, wide=False)))
    return r["o"], r["lse"].reshape(N, heads, Pq)


def raw_bwd(g, q, k, v, o, lse, heads, scale, pitched, want=ALL, null_unread=False):
    """u2pl_attn_bwd_f32 -> dict of the outputs asked for; null_unread: operands the call does not read are handed as null"""
    N, Pq, HD = q.shape
    Pk, HDv = k.shape[1], v.shape[2]
    Dh, Dv = HD // heads, HDv // heads
    gin, qin, kin, vin, oin = (Rows(t.shape, pitched, np.nan, t) for t in (g, q, k, v, o))
    lin = Rows((1, 1, N * heads * Pq), False, np.nan, np.asarray(lse, dtype=f32).reshape(1, 1, -1), wide=False)
    if null_unread and not set(want) & {"dq", "dk"}:
        vin = oin = None
    n_ws = query("u2pl_attn_bwd_ws_floats", N, heads, Pq, Pk, Dh, Dv)
    assert n_ws == B.bwd_ws_floats(N, heads, Pq, Pk, Dh, Dv)

    def run(out):
        ws = Ws(n_ws)
        call(AB, gin.ptr, gin.ld, qin.ptr, qin.ld, kin.ptr, kin.ld, *_ptr(vin), *_ptr(oin), lin.ptr, scale, N, heads, Pq, Pk, Dh, Dv,
             *_ptr(out["dq"]), *_ptr(out["dk"]), *_ptr(out["dv"]), ws.buf)
        return ws
    shapes = dict(dq=(N, Pq, HD), dk=(N, Pk, HD), dv=(N, Pk, HDv))
    return _twice("attention backward", run, lambda: {n: Rows(shapes[n], pitched, SENT) if n in want else None for n in shapes})


def saved32(q, k, v, heads, sc):
    r = B.attn_fwd64(q, k, v, heads, sc)
    return r["o"].astype(f32), r["lse"].astype(f32)


def check_case(N, heads, Pq, Pk, Dh, Dv, family, pitched, variants=False):
    """both entry points on one shape -> {output: largest error / bound}"""
    q, k, v, g = B.attn_case(N, heads, Pq, Pk, Dh, Dv, family)
    sc = B.case_scale(Dh)
    o, lse = raw_fwd(q, k, v, heads, sc, pitched)
    eo, el = B.attn_fwd_excess(o, lse, q, k, v, heads, sc)
    worst = dict(o=eo, lse=el)
    o32, l32 = saved32(q, k, v, heads, sc)
    full = raw_bwd(g, q, k, v, o32, l32, heads, sc, pitched)
    worst.update(B.attn_bwd_excess(full, g, q, k, v, o32, l32, heads, sc))
    for want in ([s for s in SUBSETS if s != ALL] if variants else []):
        got = raw_bwd(g, q, k, v, o32, l32, heads, sc, pitched, want, null_unread=True)
        assert sorted(got) == sorted(want)
        assert all(B.bits_equal(got[n], full[n]) for n in want), want          # a non-null output has the bits of the all-outputs call
    return worst


@pytest.mark.parametrize("pair", B.PAIRS, ids=lambda s: "x".join(map(str, s)))
def test_kernels_hold_the_float64_bounds(pair):
    worst = {}
    for N, heads, Dh, Dv in B.NHDD:
        worst = _merge(worst, check_case(N, heads, pair[0], pair[1], Dh, Dv, "normal", pitched=Dv in (4, 260)))
    _show("Pq = %d, Pk = %d" % pair, worst)
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("family", B.FAMILIES[1:])
def test_scores_of_100_and_a_constant_key_hold_the_bounds(family):
    worst = {}
    for c in ((3, 2, 5, 3, 20, 36), (1, 1, 33, 70, 64, 20), (3, 1, 2, 133, 4, 4)):
        worst = _merge(worst, check_case(*c, family, pitched=c[0] == 3))
    _show(family, worst)
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("family", B.ONLINE_FAMILIES)
def test_online_softmax_families_hold_the_bounds(family):
    """Pk = 16 BK + 1, Pq = BQ + 1: the row maximum in the first key tile, in the last, rising in every tile"""
    worst = check_case(1, 1, *B.ONLINE_PAIR, 4, 4, family, pitched=True)
    worst = _merge(worst, check_case(2, 2, *B.ONLINE_PAIR, 20, 8, family, pitched=False))
    _show(family, worst)
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("Pq", [B.BQ - 1, B.BQ + 1], ids=["one_tile", "two_tiles"])
def test_a_single_key_gives_its_value_row_bit_for_bit(Pq):
    q, k, v, g = B.attn_case(2, 2, Pq, 1, 8, 12)
    o, lse = raw_fwd(q, k, v, 2, 0.7, True)
    assert B.bits_equal(o, np.broadcast_to(v, o.shape).copy())


def test_every_combination_of_null_outputs():
    worst = check_case(3, 2, 70, 37, 20, 36, "normal", pitched=True, variants=True)
    worst = _merge(worst, check_case(1, 2, B.SLAB_PQ, 3, 8, 12, "normal", pitched=False, variants=True))      # two slabs
    _show("null outputs", worst)
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("case", B.GRID_CASES, ids=lambda c: "x".join(map(str, c)))
def test_first_size_past_the_grid_cap_of_every_kernel(case):
    """k_attn_fwd, k_attn_dq, k_attn_kgrad (a block per work item), k_attn_delta and k_attn_finish (256 elements a block) each take
    a second trip of their grid-stride loops in one of the cases"""
    worst = check_case(*case, "normal", pitched=False)
    _show("N, heads, Pq, Pk, D, Dv = %r" % (case,), worst)
    assert max(worst.values()) <= 1.0, worst


def test_two_runs_give_the_same_bits():
    q, k, v, g = B.attn_case(2, 3, 131, 133, 64, 260)
    sc = B.case_scale(64)
    a, b = raw_fwd(q, k, v, 3, sc, True), raw_fwd(q, k, v, 3, sc, True)
    assert B.bits_equal(a[0], b[0]) and B.bits_equal(a[1], b[1])
    x, y = (raw_bwd(g, q, k, v, a[0], a[1], 3, sc, True) for _ in range(2))
    assert all(B.bits_equal(x[n], y[n]) for n in ALL)


def test_out_of_contract_arguments_return_1001_and_leave_the_outputs_alone():
    from u2pl_amd._lib import HipError
    big = [torch.full((4096,), float(SENT), device=DEV) for _ in range(5)]
    o0, o1, o2, o3, ws = big
    src = torch.ones(4096, device=DEV)
    off = src[1:]                                                  # a base that is not 16-byte aligned

    def fwd(q=src, ldq=16, k=src, ldk=16, v=src, ldv=16, N=1, heads=2, Pq=2, Pk=3, Dm=8, Dv=8, o=o0, ldo=16, lse=o1, ws_=ws):
        return (AF, q, ldq, k, ldk, v, ldv, 0.5, N, heads, Pq, Pk, Dm, Dv, o, ldo, lse, ws_)

    def bwd(g=src, ldg=16, q=src, ldq=16, k=src, ldk=16, v=src, ldv=16, o=src, ldo=16, lse=src, N=1, heads=2, Pq=2, Pk=3, Dm=8, Dv=8,
            dq=o0, lddq=16, dk=o1, lddk=16, dv=o2, lddv=16, ws_=ws):
        return (AB, g, ldg, q, ldq, k, ldk, v, ldv, o, ldo, lse, 0.5, N, heads, Pq, Pk, Dm, Dv, dq, lddq, dk, lddk, dv, lddv, ws_)
    bad = [fwd(N=0), fwd(heads=0), fwd(Pq=0), fwd(Pk=0), fwd(Dm=0), fwd(Dm=6), fwd(Dm=132, ldq=264, ldk=264), fwd(Dv=0), fwd(Dv=6),
           fwd(Dv=516, ldv=1032, ldo=1032), fwd(N=2 ** 20, Pq=2 ** 11), fwd(N=2 ** 20, Pk=2 ** 11), fwd(N=2 ** 19, Pq=2 ** 11),
           fwd(q=None), fwd(k=None), fwd(v=None), fwd(o=None), fwd(lse=None),
           fwd(ldq=12), fwd(ldk=18), fwd(ldv=12), fwd(ldo=17), fwd(q=off), fwd(v=off), fwd(o=off),
           bwd(N=0), bwd(heads=0), bwd(Pq=0), bwd(Pk=0), bwd(Dm=6), bwd(Dv=6), bwd(Dm=132, ldq=264, ldk=264, lddq=264, lddk=264),
           bwd(g=None), bwd(q=None), bwd(k=None), bwd(lse=None), bwd(ws_=None), bwd(v=None), bwd(o=None), bwd(v=None, dk=None),
           bwd(dq=None, dk=None, dv=None),                                     # no output asked for
           bwd(ldg=12), bwd(ldq=18), bwd(ldk=12), bwd(ldv=12), bwd(ldo=12), bwd(lddq=12), bwd(lddk=18), bwd(lddv=12),
           bwd(g=off), bwd(dv=off), bwd(dq=off), bwd(ws_=off)]
    for args in bad:
        with pytest.raises(HipError, match="1001"):
            call(*args)
    torch.cuda.synchronize()
    assert all(bool((o.view(torch.int32) == B.SENTINEL_BITS).all()) for o in big)
    assert query("u2pl_attn_bwd_ws_floats", 1, 2, 2, 3, 6, 8) == 0 and query("u2pl_attn_bwd_ws_floats", 1, 2, 2, 3, 8, 516) == 0
    assert query("u2pl_attn_bwd_ws_floats", 1, 2, 2, 3, 8, 8) == 4 and query("u2pl_attn_fwd_ws_floats", 1, 2, 2, 3, 8, 8) == 0
    call(*fwd())                                                   # the base case of the list is in contract
    call(*bwd())
    call(*fwd(ws_=None))                                           # the forward's workspace query is 0: a null ws is in contract
    call(*bwd(v=None, o=None, dq=None, dk=None))                   # v and o are not read for dv alone
    torch.cuda.synchronize()


# ---- the autograd Function ----------------------------------------------------------------------------------------------------
def act(a, hw):
    """[N, P, C] numpy -> channels_last [N, C, H, W] on the device"""
    return D(a).reshape(a.shape[0], hw[0], hw[1], a.shape[2]).permute(0, 3, 1, 2)


def rows_of(t):
    """[N, C, H, W] tensor -> [N, H W, C] numpy"""
    return t.detach().permute(0, 2, 3, 1).flatten(1, 2).contiguous().cpu().numpy()


@pytest.mark.parametrize("N,heads,Dh,Dv,hwq,hwk", [(3, 2, 20, 36, (7, 10), (7, 10)), (1, 1, 64, 4, (2, 3), (2, 3)), (2, 3, 8, 132, (13, 21), (7, 11))],
                         ids=["7x10", "2x3", "13x21_keys_7x11"])
def test_function_gives_the_bits_of_the_raw_calls(N, heads, Dh, Dv, hwq, hwk):
    from u2pl_amd import nn as Kn
    Pq, Pk = hwq[0] * hwq[1], hwk[0] * hwk[1]
    q, k, v, g = B.attn_case(N, heads, Pq, Pk, Dh, Dv)
    sc = B.case_scale(Dh)
    qd, kd, vd = (t.requires_grad_(True) for t in (act(q, hwq), act(k, hwk), act(v, hwk)))
    gd = act(g, hwq)
    with recorded_calls(Kn) as seen:
        out = Kn.dense_attention(qd, kd, vd, heads=heads, scale=sc)
        out.backward(gd)
    torch.cuda.synchronize()
    assert {n: len(a) for n, a in seen.items()} == {AF: 1, AB: 1}
    assert seen[AF][0][7:13] == (N, heads, Pq, Pk, Dh, Dv)
    o, lse = raw_fwd(q, k, v, heads, sc, False)
    assert out.shape == (N, heads * Dv) + hwq and B.bits_equal(rows_of(out), o)
    got = raw_bwd(g, q, k, v, o, lse, heads, sc, False)
    assert B.bits_equal(rows_of(qd.grad), got["dq"]) and B.bits_equal(rows_of(kd.grad), got["dk"]) and B.bits_equal(rows_of(vd.grad), got["dv"])
    assert qd.grad.shape == qd.shape and kd.grad.shape == kd.shape and vd.grad.shape == vd.shape
    # nothing needs a gradient: no backward node; scale None is D ** -0.5
    with recorded_calls(Kn) as seen:
        y = Kn.dense_attention(qd.detach(), kd.detach(), vd.detach(), heads=heads)
    assert y.grad_fn is None and seen[AF][0][6] == float(Dh) ** -0.5 and AB not in seen
    # only k needs a gradient: dq and dv are null outputs
    kd.grad = None
    with recorded_calls(Kn) as seen:
        Kn.dense_attention(qd.detach(), kd, vd.detach(), heads=heads, scale=sc).backward(gd)
    a = seen[AB][0]
    assert a[18] is None and a[22] is None and a[20] is not None
    assert B.bits_equal(rows_of(kd.grad), got["dk"])
    # only v needs one
    vd.grad = None
    with recorded_calls(Kn) as seen:
        Kn.dense_attention(qd.detach(), kd.detach(), vd, heads=heads, scale=sc).backward(gd)
    a = seen[AB][0]
    assert a[18] is None and a[20] is None and a[22] is not None and B.bits_equal(rows_of(vd.grad), got["dv"])


def test_shapes_are_checked_before_any_call():
    from u2pl_amd import nn as Kn
    z = lambda *s: torch.zeros(*s, device=DEV)      # noqa: E731
    with recorded_calls(Kn) as seen:
        for q, k, v, heads in ((z(1, 6, 2, 2), z(1, 6, 2, 2), z(1, 8, 2, 2), 1), (z(1, 8, 2, 2), z(1, 8, 2, 2), z(1, 6, 2, 2), 1),
                               (z(1, 8, 2, 2), z(1, 8, 2, 3), z(1, 8, 2, 2), 1), (z(1, 8, 2, 2), z(1, 4, 2, 2), z(1, 8, 2, 2), 1),
                               (z(2, 8, 2, 2), z(1, 8, 2, 2), z(1, 8, 2, 2), 1), (z(1, 8, 2, 2), z(1, 8, 2, 2), z(1, 8, 2, 2), 3),
                               (z(1, 8, 2, 2), z(1, 8, 2, 2), z(1, 8, 2, 2), 4), (z(1, 8, 2, 2), z(1, 8, 2, 2), z(1, 12, 2, 2), 2),
                               (z(1, 132, 2, 2), z(1, 132, 2, 2), z(1, 8, 2, 2), 1), (z(1, 8, 2, 2), z(1, 8, 2, 2), z(1, 516, 2, 2), 1),
                               (z(1, 8, 2, 2), z(1, 8, 2, 2), z(1, 8, 2, 2), 0)):
            with pytest.raises(ValueError):
                Kn.dense_attention(q, k, v, heads=heads)
    assert not seen


# ---- the decoder against its float64 twin -------------------------------------------------------------------------------------
def _nl_twin(dec, p, x):
    f = _seq64(dec.conva, p, "conva", x)
    b = dec.nl
    q = F.conv2d(f, p["nl.query.weight"], p["nl.query.bias"])
    k = F.conv2d(f, p["nl.key.weight"], p["nl.key.bias"], stride=b.key.stride)
    v = F.conv2d(f, p["nl.value.weight"], p["nl.value.bias"], stride=b.value.stride)
    N, _, H, W = q.shape
    qh, kh, vh = (B.hd(t.flatten(2).transpose(1, 2), b.heads) for t in (q, k, v))
    sc = float(qh.shape[3]) ** -0.5 if b.scale is None else b.scale
    o = B.un(torch.softmax(sc * (qh @ kh.transpose(2, 3)), 3) @ vh).transpose(1, 2).reshape(N, -1, H, W)
    f = f + _seq64(b.project, p, "nl.project", o)
    out = _seq64(dec.bottleneck, p, "bottleneck", torch.cat((x, _seq64(dec.convb, p, "convb", f)), 1))
    return dict(pred=F.conv2d(out, p["classifier.weight"], p["classifier.bias"]), rep=_seq64(dec.representation, p, "representation", out))


# the key's bias adds q[p] . b to EVERY score of the query p, which the softmax does not see: its exact gradient is zero.  The
# value's bias is the same case: the weights of a query sum to 1, so it adds one constant per channel to the block's projection,
# which the train-mode BatchNorm behind it subtracts with the mean.  (Zero but for float64 roundings of sums of the weight's size.)
KEY_AND_VALUE_BIAS_ARE_ZERO = ((".key.bias", ".value.bias"), lambda scale, wsum: scale <= 1e-10 * wsum)


@pytest.mark.parametrize("kv_stride,heads", [(1, 1), (2, 2), (2, 1), (1, 2)])
def test_nonlocal_decoder_is_no_worse_than_the_deeplabv3_decoder(kv_stride, heads):
    """(figures re-draws every norm's affine pair: the block's zero-initialised norm weight too, so the attention is live)"""
    from u2pl_amd.models.decoder import dec_nonlocal
    assert_no_worse_than_deeplabv3(
        "dec_nonlocal", lambda: dec_nonlocal(in_planes=128, inner_planes=64, key_planes=32, value_planes=48, heads=heads,
                                             kv_stride=kv_stride, rep_head=True), _nl_twin, ("pred", "rep"),
        {"pred", "rep", "dx", "conva.0.weight", "nl.query.weight", "nl.key.bias", "nl.value.weight", "nl.project.0.weight", "nl.project.1.weight",
         "convb.0.weight", "bottleneck.0.weight", "classifier.bias", "representation.4.weight"}, zero_grad=KEY_AND_VALUE_BIAS_ARE_ZERO)


# ---- the whole path -----------------------------------------------------------------------------------------------------------
NL_DECODER = dict(type="u2pl.models.decoder.dec_nonlocal", kwargs=dict(rep_head=True))


@pytest.fixture(scope="module")
def nlnet():
    return build_net(decoder_cfg(NL_DECODER)), net_input()


QKV = ["decoder.nl.%s.weight" % n for n in ("query", "key", "value")]


def test_nonlocal_train_step_reaches_every_parameter_and_the_norm_weight_leaves_zero(nlnet):
    from u2pl_amd import nn as Kn
    model, x = nlnet
    model.train()
    w0 = model.decoder.nl.project[1].weight
    assert not bool(w0.detach().any())
    before = {n_: p.detach().clone() for n_, p in model.named_parameters() if n_ in QKV}
    opt = torch.optim.SGD(model.parameters(), lr=1e-3)
    opt.zero_grad(set_to_none=True)
    seen, outs = step_calls(model, x)
    assert sorted(outs) == ["aux", "pred", "rep"] and outs["pred"].shape == (4, 19, 9, 9)
    assert [len(seen[n_]) for n_ in (AF, AB)] == [1, 1]
    assert seen[AF][0][7:13] == (4, 1, 81, 81, 64, 256) and seen[AF][0][6] == 0.125
    missing = [n_ for n_, p in model.named_parameters() if p.grad is None]
    assert not missing, missing
    assert not [n_ for n_, p in model.named_parameters() if not bool(torch.isfinite(p.grad).all())]
    # at a zero norm weight the gradients of q, k and v are exactly zero: what moves first is the norm weight
    params = dict(model.named_parameters())
    assert all(not bool(params[n_].grad.any()) for n_ in QKV) and bool(w0.grad.ne(0).any())
    opt.step()
    Kn.invalidate_weights()
    assert bool(w0.detach().ne(0).any())                                        # after the first SGD step it has left 0
    assert all(torch.equal(params[n_].detach(), before[n_]) for n_ in QKV)
    opt.zero_grad(set_to_none=True)
    step_calls(model, x)                                                        # the attention is live now: every parameter moves
    bad = [n_ for n_, p in model.named_parameters() if not bool(torch.isfinite(p.grad).all())]
    # (the key's and the value's bias have a zero gradient in exact arithmetic: KEY_AND_VALUE_BIAS_ARE_ZERO)
    zero = [n_ for n_, p in model.named_parameters() if not bool(p.grad.ne(0).any()) and not n_.endswith(("nl.key.bias", "nl.value.bias"))]
    assert not bad and not zero, (bad, zero)
    opt.step()
    Kn.invalidate_weights()
    assert all(not torch.equal(params[n_].detach(), before[n_]) for n_ in QKV)  # after the second step q, k and v have moved
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())


def test_nonlocal_eval_forward_is_the_same_with_and_without_a_graph(nlnet):
    assert_eval_forward_ignores_the_graph(nlnet)


def test_default_config_makes_no_attn_call_and_the_same_calls_after_a_nonlocal_step(nlnet):
    assert_default_config_is_untouched(nlnet, AF, "u2pl_attn_")


def test_nonlocal_graph_replay_is_bit_identical_to_eager(monkeypatch):
    """two heads over strided keys; the block's norm weight starts at 0 and SGD moves it between the steps"""
    two_heads = dict(type=NL_DECODER["type"], kwargs=dict(rep_head=True, kv_stride=2, heads=2))
    a, b = (train_steps(monkeypatch, on, lambda cfg: cfg["net"].update(decoder=two_heads),
                        probe=lambda model: float(model.decoder.nl.project[1].weight.detach().abs().sum())) for on in (True, False))
    print("graph stats", a["stats"], "|norm weight| after each step", a["probes"])
    assert_replay_equals_eager(a, b)
    assert a["probes"][0] != 0.0 and len(set(a["probes"])) == len(a["probes"])         # the norm weight moves at every step
    assert a["probes"] == b["probes"]


# ---- prediction ----------------------------------------------------------------------------------------------------------------
def test_infer_image_runs_on_a_map_that_the_criss_cross_decoder_refuses(nlnet):
    """at stride 8 a 9 x 4089 input is a 2 x 512 map: H + W - 1 = 513 > CC_MAX_L, 1024 queries against 1024 keys here"""
    from u2pl_amd import infer as I
    from u2pl_amd import nn as Kn
    model, _ = nlnet
    model.eval()
    try:
        lut = torch.from_numpy(I.normalise_lut([123.675, 116.28, 103.53], [58.395, 57.12, 57.375])).to(DEV)
        img = torch.randint(0, 256, (9, 64, 3), generator=torch.Generator().manual_seed(4), dtype=torch.uint8).to(DEV)
        with pytest.raises(ValueError, match="too large for one cross"):
            Kn.check_cc_shapes(1, 2, 512, 64, 512)
        with recorded_calls(Kn) as seen:
            label, _, pred = I.infer_image(model, img, lut, (9, 4089))[:3]
        torch.cuda.synchronize()
        assert seen[AF][0][7:11] == (1, 1, 1024, 1024) and AB not in seen
        assert label.shape == (9, 64) and bool(torch.isfinite(pred).all())
    finally:
        model.train()
