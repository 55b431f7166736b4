"""Dense attention and dec_nonlocal without a GPU: the float64 references of tests/attn_bounds.py are torch's float64 autograd of
the dense formula (and agree with F.scaled_dot_product_attention); the numpy fp32 emulation of the kernels' own order meets its
bounds on every table shape; the named faulty emulations leave them; the calibrated ceilings are re-measured from torch's own
fp32 arithmetic (-s -k ceilings prints them); check_attn_shapes refuses what the entry points refuse; dec_nonlocal builds with
the documented keys, refuses what it documents, starts as the identity and routes its inputs.  (The HIP kernels are held to the
same bounds in tests/test_gpu_attn.py.)"""
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_bounds as B  # noqa: E402
from model_utils import net_cfg  # noqa: E402
from u2pl_amd import nn as K  # noqa: E402
from u2pl_amd.models.decoder import NonLocalBlock, dec_ccnet, dec_nonlocal  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATTN_HIP = open(os.path.join(ROOT, "u2pl_amd", "csrc", "attn.hip")).read()      # the kernels this file's emulations restate
f32, f64 = np.float32, np.float64
ALL_FAMILIES = B.FAMILIES + B.ONLINE_FAMILIES
REF_SHAPES = ((1, 1, 1, 1, 4, 4), (2, 2, 3, 5, 4, 8), (2, 3, 7, 1, 8, 4), (1, 1, 1, 7, 4, 4), (2, 2, 9, 70, 20, 12))
FAULT = dict(N=2, heads=2, Pq=70, Pk=133, D=8, Dv=12)      # Pq, Pk no multiples of 16, three key tiles, two heads
SLAB_FAULT = dict(N=1, heads=2, Pq=B.SLAB_PQ, Pk=3, D=8, Dv=12)


def _saved(q, k, v, heads, sc):
    r = B.attn_fwd64(q, k, v, heads, sc)
    return r["o"].astype(f32), r["lse"].astype(f32)


# ------------------------------------------------------------------ the references are torch's float64 autograd
@pytest.mark.parametrize("family", ALL_FAMILIES)
def test_plain_formulas_are_torchs_autograd_of_the_dense_attention_in_float64(family):
    for N, H, Pq, Pk, D, Dv in REF_SHAPES:
        q, k, v, g = B.attn_case(N, H, Pq, Pk, D, Dv, family)
        sc = B.case_scale(D)
        d = B.dense64(q, k, v, H, sc, g)
        r = B.attn_fwd64(q, k, v, H, sc)
        assert np.abs(r["o"] - d["o"]).max() <= 1e-13 * max(r["unit_o"].max(), 1.0)
        assert np.abs(r["lse"] - d["lse"]).max() <= 1e-12 * (1 + np.abs(d["lse"]).max())
        assert (r["unit_o"] >= np.abs(r["o"]) - 1e-12 * r["unit_o"].max()).all()
        b = B.attn_bwd64(g, q, k, v, d["o"], d["lse"], H, sc)
        for n in B.OUTS_BWD:
            assert np.abs(b[n] - d[n]).max() <= 1e-11 * max(b["unit_" + n].max(), 1e-300), n
            assert (b["unit_" + n] >= np.abs(b[n]) - 1e-9 * b["unit_" + n].max()).all(), n


@pytest.mark.parametrize("family", ALL_FAMILIES)
def test_scaled_dot_product_attention_in_float64_agrees_with_the_reference(family):
    for N, H, Pq, Pk, D, Dv in REF_SHAPES:
        q, k, v, g = B.attn_case(N, H, Pq, Pk, D, Dv, family)
        sc = B.case_scale(D)
        qt, kt, vt = (B.hd(B.T(t, torch.float64), H).requires_grad_(True) for t in (q, k, v))
        o = F.scaled_dot_product_attention(qt, kt, vt, scale=float(f32(sc)))
        (o * B.hd(B.T(g, torch.float64), H)).sum().backward()
        d = B.dense64(q, k, v, H, sc, g)
        for got, n in ((o.detach(), "o"), (qt.grad, "dq"), (kt.grad, "dk"), (vt.grad, "dv")):
            assert np.abs(B.un(got).numpy() - d[n]).max() <= 1e-11 * max(np.abs(d[n]).max(), 1.0), n


def test_online_families_put_the_row_maximum_where_they_say():
    Pq, Pk = B.ONLINE_PAIR
    assert Pk == 16 * B.BK + 1 and Pq == B.BQ + 1
    for fam in B.ONLINE_FAMILIES:
        q, k, v, g = B.attn_case(1, 1, Pq, Pk, 4, 4, fam)
        u = B._scores64(q, k, 1, B.case_scale(4))[0][0, 0]
        tile_max = np.stack([u[:, t:t + B.BK].max(1) for t in range(0, Pk, B.BK)], 1)
        run = np.maximum.accumulate(tile_max, 1)
        if fam == "first":
            assert (u.argmax(1) < B.BK).all() and (run[:, 1:] == run[:, :1]).all()
        elif fam == "last":
            assert (u.argmax(1) == Pk - 1).all()
        else:
            assert (np.diff(u, axis=1) > 0).all() and (np.diff(run, axis=1) > 0).all()     # every tile raises the maximum


# ------------------------------------------------------------------ the tables and the constants mirror the kernel file
def test_constants_mirror_the_kernel_file():
    for name, val in (("ATTN_BQ", B.BQ), ("ATTN_BK", B.BK), ("ATTN_DVC", B.DVC), ("ATTN_MAX_D", B.MAX_D), ("ATTN_MAX_DV", B.MAX_DV),
                      ("ATTN_MAX_BLOCKS", B.GRID_CAP), ("ATTN_FILL", B.FILL), ("ATTN_SLAB_MIN", B.SLAB_MIN), ("ATTN_MAX_SLABS", B.MAX_SLABS)):
        m = re.search(r"#define %s (\d+)" % name, ATTN_HIP)
        assert m and int(m.group(1)) == val, name
    assert (K.ATTN_MAX_D, K.ATTN_MAX_DV) == (B.MAX_D, B.MAX_DV)
    assert "ARITHMETIC CONTRACT" in ATTN_HIP and "__builtin_amdgcn_mfma_f32_16x16x4f32" in ATTN_HIP
    assert not re.search(r"atomic|hipMemset", ATTN_HIP.split("#include")[1])
    pairs = set(B.PAIRS)
    assert {(1, 1), (1, 7), (7, 1), (3, 5), (B.BQ - 1, B.BK - 1), (B.BQ, B.BK), (B.BQ + 1, B.BK + 1), (2 * B.BQ + 3, 2 * B.BK + 5),
            (B.BQ + 1, 1), (1, 2 * B.BK + 5), (B.SLAB_PQ, 3)} == pairs
    assert set(B.NHDD) == {(1, 1, 4, 4), (1, 1, 128, 4), (3, 2, 20, 36), (2, 3, 64, 260), (1, 1, 64, 512)}
    for N, H, _, _ in B.NHDD:                                   # SLAB_PQ is the first Pq with a second slab in every row of the table
        assert B.slabs(N, H, B.SLAB_PQ, 3)[0] == 2 and B.slabs(N, H, B.SLAB_PQ - 1, 3)[0] == 1
    assert B.slabs(4, 1, 97 * 97, 97 * 97) == (1, 9472) and B.slabs(4, 1, 97 * 97, 49 * 49)[0] == 4
    assert B.bwd_ws_floats(1, 1, 5, 3, 4, 8) == 8 and B.bwd_ws_floats(1, 2, B.SLAB_PQ, 3, 4, 8) == 516 + 2 * 3 * 2 * 12


def test_tile_order_is_the_permutation_of_an_mfma_step():
    order = B.tile_order(64)
    assert sorted(order) == list(range(64)) and order[:8] == [0, 4, 8, 12, 1, 5, 9, 13] and order[16:20] == [16, 20, 24, 28]
    assert B.tile_order(64, natural=True) == list(range(64))
    assert B.tile_order(6) == [0, 4, 1, 5, 2, 3]


# ------------------------------------------------------------------ the faithful emulation holds every bound
def _emu_worst(N, H, Pq, Pk, D, Dv, family):
    q, k, v, g = B.attn_case(N, H, Pq, Pk, D, Dv, family)
    sc = B.case_scale(D)
    o, lse = B.emu_fwd(q, k, v, H, sc)
    eo, el = B.attn_fwd_excess(o, lse, q, k, v, H, sc)
    o32, l32 = _saved(q, k, v, H, sc)
    worst = dict(o=eo, lse=el, **B.attn_bwd_excess(B.emu_bwd(g, q, k, v, o32, l32, H, sc), g, q, k, v, o32, l32, H, sc))
    return worst


@pytest.mark.parametrize("pair", B.PAIRS, ids=lambda s: "x".join(map(str, s)))
def test_faithful_emulation_holds_every_bound_at_every_table_shape(pair):
    for N, H, D, Dv in B.NHDD:
        worst = _emu_worst(N, H, pair[0], pair[1], D, Dv, "normal")
        assert max(worst.values()) <= 1.0, (pair, N, H, D, Dv, worst)


@pytest.mark.parametrize("family", ALL_FAMILIES)
def test_faithful_emulation_holds_every_bound_in_every_score_family(family):
    cases = [(3, 2, 5, 3, 20, 36), (1, 1, 33, 70, 64, 20), (3, 1, 2, 133, 4, 4)]
    if family in B.ONLINE_FAMILIES:
        cases = [(1, 1) + B.ONLINE_PAIR + (4, 4), (2, 2) + B.ONLINE_PAIR + (20, 8)]
    for c in cases:
        worst = _emu_worst(*c, family)
        assert max(worst.values()) <= 1.0, (c, worst)


def test_single_key_gives_the_value_row_bit_for_bit():
    for Pq in (B.BQ - 1, B.BQ + 1):
        q, k, v, g = B.attn_case(2, 2, Pq, 1, 8, 12)
        o, lse = B.emu_fwd(q, k, v, 2, 0.7)
        assert B.bits_equal(o, np.broadcast_to(v, o.shape).copy())


# ------------------------------------------------------------------ the faulty emulations leave the bounds
def _fault_case(c, family="normal"):
    q, k, v, g = B.attn_case(c["N"], c["heads"], c["Pq"], c["Pk"], c["D"], c["Dv"], family)
    return q, k, v, g, B.case_scale(c["D"])


@pytest.mark.parametrize("fault", [f for f in B.FAULTS_FWD if f != "rows_past_pq"])
def test_faulty_forward_emulations_break_a_bound(fault):
    family = "ascending" if fault == "no_rescale" else "normal"
    q, k, v, g, sc = _fault_case(FAULT, family)
    H = FAULT["heads"]
    assert max(B.attn_fwd_excess(*B.emu_fwd(q, k, v, H, sc), q, k, v, H, sc)) <= 1.0
    assert max(B.attn_fwd_excess(*B.emu_fwd(q, k, v, H, sc, fault), q, k, v, H, sc)) > 1.0


def test_query_rows_past_the_last_are_caught_by_the_sentinel_frame():
    q, k, v, g, sc = _fault_case(FAULT)
    H, Pq = FAULT["heads"], FAULT["Pq"]
    assert Pq % 16
    assert B.frame_intact(B.emu_fwd(q, k, v, H, sc)[0], Pq)
    assert not B.frame_intact(B.emu_fwd(q, k, v, H, sc, "rows_past_pq")[0], Pq)


@pytest.mark.parametrize("fault", B.FAULTS_BWD)
def test_faulty_backward_emulations_break_a_bound(fault):
    c = SLAB_FAULT if fault == "last_slab_dropped" else FAULT
    q, k, v, g, sc = _fault_case(c)
    H = c["heads"]
    assert B.slabs(c["N"], H, c["Pq"], c["Pk"])[0] == (2 if c is SLAB_FAULT else 1)
    o32, l32 = _saved(q, k, v, H, sc)
    good = B.attn_bwd_excess(B.emu_bwd(g, q, k, v, o32, l32, H, sc), g, q, k, v, o32, l32, H, sc)
    bad = B.attn_bwd_excess(B.emu_bwd(g, q, k, v, o32, l32, H, sc, fault), g, q, k, v, o32, l32, H, sc)
    assert max(good.values()) <= 1.0, good
    assert max(bad.values()) > 1.0, bad


def test_there_are_at_least_ten_faults():
    assert len(set(B.FAULTS_FWD) | set(B.FAULTS_BWD)) >= 10


# ------------------------------------------------------------------ the ceilings
def test_ceilings_are_what_torchs_fp32_arithmetic_reaches():
    meas, emu = B.measure("torch"), B.measure("emu")
    print("\nmeasured (torch fp32 / emulation), in EPS (1 + arg) unit:")
    for n in B.CAL:
        print("   %-4s %.3f [%.3f]   ceiling %.3f" % (n, meas[n], emu[n], B.CAL[n]))
    for n in B.CAL:
        assert meas[n] <= B.CAL[n] <= 2 * meas[n] + 1e-12, (n, meas[n], B.CAL[n])
        assert emu[n] <= B.CAL_MARGIN * B.CAL[n], (n, emu[n])


# ------------------------------------------------------------------ check_attn_shapes
def test_check_attn_shapes_refuses_what_the_entry_points_refuse():
    assert K.check_attn_shapes(4, 1, 97 * 97, 49 * 49, 64, 256) == (4, 1, 9409, 2401, 64, 256)
    assert K.check_attn_shapes(1, 8, 1, 1, 128, 512) == (1, 8, 1, 1, 128, 512)
    for bad in ((0, 1, 1, 1, 4, 4), (1, 0, 1, 1, 4, 4), (1, 1, 0, 1, 4, 4), (1, 1, 1, 0, 4, 4)):
        with pytest.raises(ValueError, match=">= 1"):
            K.check_attn_shapes(*bad)
    for D in (0, 2, 6, 132):
        with pytest.raises(ValueError, match=r"key channels per head.*4 \.\. 128"):
            K.check_attn_shapes(1, 1, 1, 1, D, 4)
    for Dv in (0, 2, 6, 516):
        with pytest.raises(ValueError, match=r"value channels per head.*4 \.\. 512"):
            K.check_attn_shapes(1, 1, 1, 1, 4, Dv)
    for bad in ((2, 1, 2 ** 30, 1, 4, 4), (1, 2, 2 ** 30, 1, 4, 4), (2, 1, 1, 2 ** 30, 4, 4)):
        with pytest.raises(ValueError, match=r"2\^31"):
            K.check_attn_shapes(*bad)
    with pytest.raises(ValueError, match="my layer"):
        K.check_attn_shapes(1, 1, 1, 1, 3, 4, what="my layer")


def test_header_declares_the_entry_points_with_a_contract_block():
    head = open(os.path.join(ROOT, "include", "u2pl_hip.h")).read()
    for name in ("u2pl_attn_fwd_ws_floats", "u2pl_attn_fwd_f32", "u2pl_attn_bwd_ws_floats", "u2pl_attn_bwd_f32"):
        assert re.search(r"\b%s\(" % name, head), name
    assert "CONTRACT.  1001 before any launch" in head.split("u2pl_attn_fwd_ws_floats")[0].rsplit("/*", 1)[1]


# ------------------------------------------------------------------ dec_nonlocal
def nl_keys(in_planes=2048, num_classes=19, inner=512, key=64, value=256, rep=False):
    keys = {}

    def bn(prefix, c):
        keys.update({prefix + ".weight": (c,), prefix + ".bias": (c,), prefix + ".running_mean": (c,),
                     prefix + ".running_var": (c,), prefix + ".num_batches_tracked": ()})

    def unit3(prefix, cin, cout):
        keys[prefix + ".0.weight"] = (cout, cin, 3, 3)
        bn(prefix + ".1", cout)
    unit3("conva", in_planes, inner)
    for name, cout in (("query", key), ("key", key), ("value", value)):
        keys.update({"nl.%s.weight" % name: (cout, inner, 1, 1), "nl.%s.bias" % name: (cout,)})
    keys["nl.project.0.weight"] = (inner, value, 1, 1)
    bn("nl.project.1", inner)
    unit3("convb", inner, inner)
    unit3("bottleneck", in_planes + inner, inner)
    keys.update({"classifier.weight": (num_classes, inner, 1, 1), "classifier.bias": (num_classes,)})
    if rep:
        keys["representation.0.weight"] = (256, inner, 3, 3)
        bn("representation.1", 256)
        keys.update({"representation.4.weight": (256, 256, 1, 1), "representation.4.bias": (256,)})
    return keys


@pytest.mark.parametrize("rep", [False, True])
def test_dec_nonlocal_builds_with_the_documented_keys_and_a_zero_norm_weight(rep):
    dec = dec_nonlocal(in_planes=2048, rep_head=rep)
    assert {k: tuple(v.shape) for k, v in dec.state_dict().items()} == nl_keys(rep=rep)
    assert isinstance(dec.bottleneck[3], torch.nn.Dropout2d) and dec.bottleneck[3].p == 0.1
    w = dec.nl.project[1].weight
    assert not bool(w.detach().any()) and w.requires_grad                     # the paper's initialisation: the identity at step 0
    assert bool((dec.conva[1].weight.detach() == 1).all())                    # every other norm keeps its own
    assert (dec.nl.key.stride, dec.nl.value.stride, dec.nl.query.stride) == (1, 1, 1) and dec.nl.heads == 1 and dec.nl.scale is None
    dec = dec_nonlocal(in_planes=96, num_classes=150, inner_planes=64, key_planes=8, value_planes=1024, heads=2, kv_stride=2,
                       scale=0.3, rep_head=rep)
    assert {k: tuple(v.shape) for k, v in dec.state_dict().items()} == nl_keys(96, 150, 64, 8, 1024, rep)
    assert (dec.nl.key.stride, dec.nl.value.stride, dec.nl.query.stride) == (2, 2, 1) and dec.nl.heads == 2 and dec.nl.scale == 0.3
    assert dec.nl.key.bias is not None and dec.nl.value.bias is not None and dec.nl.project[0].bias is None


def test_dec_nonlocal_refuses_what_it_documents():
    for kw in (dict(in_planes=2046), dict(in_planes=2048, inner_planes=510), dict(in_planes=2048, key_planes=30),
               dict(in_planes=2048, value_planes=0)):
        with pytest.raises(ValueError, match="multiple of 4"):
            dec_nonlocal(**kw)
    for kw in (dict(heads=0), dict(heads=3), dict(key_planes=64, value_planes=260, heads=8)):
        with pytest.raises(ValueError, match="divide into heads"):
            dec_nonlocal(in_planes=2048, **kw)
    with pytest.raises(ValueError, match="key channels per head"):
        dec_nonlocal(in_planes=2048, key_planes=256)
    with pytest.raises(ValueError, match="key channels per head"):
        dec_nonlocal(in_planes=2048, key_planes=8, value_planes=8, heads=4)   # 2 per head
    with pytest.raises(ValueError, match="value channels per head"):
        dec_nonlocal(in_planes=2048, value_planes=1024)
    for s in (0, 3, 4):
        with pytest.raises(ValueError, match="kv_stride"):
            dec_nonlocal(in_planes=2048, kv_stride=s)
    for nc in (0, 1, 256):
        with pytest.raises(ValueError, match="num_classes"):
            dec_nonlocal(in_planes=2048, num_classes=nc)
    with pytest.raises(TypeError):
        dec_nonlocal(in_planes=2048, separable=True)
    dec_nonlocal(in_planes=48, num_classes=255, inner_planes=8, key_planes=256, value_planes=1024, heads=2)   # 128 and 512 per head


def test_other_decoders_keep_their_keys():
    sd = dec_ccnet(in_planes=2048).state_dict()
    assert "cca.gamma" in sd and not [k for k in sd if k.startswith("nl.")]


def test_dec_nonlocal_resolves_through_the_alias_package_and_the_default_config_builds_what_it_built():
    import importlib
    from u2pl_amd.models.model_helper import ModelBuilder
    assert importlib.import_module("u2pl.models.decoder").dec_nonlocal is dec_nonlocal
    cfg = net_cfg("resnet50", 19, True)
    default = ModelBuilder(net_cfg("resnet50", 19, True))
    assert type(default.decoder).__name__ != "dec_nonlocal" and not [k for k in default.state_dict() if ".nl." in k]
    cfg["decoder"] = dict(type="u2pl.models.decoder.dec_nonlocal", kwargs=dict(rep_head=True, kv_stride=2, heads=2))
    model = ModelBuilder(cfg)
    assert isinstance(model.decoder, dec_nonlocal) and isinstance(model.decoder.nl, NonLocalBlock)
    sd = model.state_dict()
    assert tuple(sd["decoder.conva.0.weight"].shape) == (512, 2048, 3, 3)
    assert tuple(sd["decoder.nl.key.weight"].shape) == (64, 512, 1, 1) and tuple(sd["decoder.nl.project.0.weight"].shape) == (512, 256, 1, 1)
    assert tuple(sd["decoder.bottleneck.0.weight"].shape) == (512, 2560, 3, 3)
    assert tuple(sd["decoder.representation.4.weight"].shape) == (256, 256, 1, 1)
    assert tuple(sd["auxor.aux.0.weight"].shape) == (256, 1024, 3, 3)
    enc = {k: tuple(v.shape) for k, v in sd.items() if k.startswith("encoder.")}
    assert enc == {k: tuple(v.shape) for k, v in default.state_dict().items() if k.startswith("encoder.")}


def _torch_ops(monkeypatch):
    """the decoder's wiring without a GPU: every u2pl_amd.nn operation it calls replaced by the torch function it stands for, and
    the attention calls recorded (the HIP operations themselves are tests/test_gpu_attn.py's)"""
    seen = []

    def conv(m, x):
        return F.conv2d(x, m.weight, m.bias, stride=m.stride, padding=m.padding)

    def bn(m, x):
        return F.batch_norm(x, None, None, m.weight, m.bias, training=True)

    def seq(s, x):
        for m in s:
            if isinstance(m, K.Conv2d):
                x = conv(m, x)
            elif isinstance(m, K.BatchNorm2d):
                x = bn(m, x)
            elif isinstance(m, torch.nn.ReLU):
                x = torch.relu(x)
        return x

    def attention(q, k, v, heads=1, scale=None):
        seen.append((tuple(q.shape), tuple(k.shape), tuple(v.shape), heads, scale))
        N, _, Hq, Wq = q.shape
        qh, kh, vh = (B.hd(t.flatten(2).transpose(1, 2), heads) for t in (q, k, v))
        o = F.scaled_dot_product_attention(qh, kh, vh, scale=scale)
        return B.un(o).transpose(1, 2).reshape(N, -1, Hq, Wq)

    monkeypatch.setattr(K, "dense_attention", attention)
    monkeypatch.setattr(K, "cat_channels", lambda ts: torch.cat(tuple(ts), 1))
    monkeypatch.setattr(K, "run_seq", lambda s, x, grad_link=None: seq(s, x))
    monkeypatch.setattr(K, "conv_bn", lambda c, b, x, res=None, relu=False: bn(b, conv(c, x)) + res)
    monkeypatch.setattr(K.Conv2d, "forward", lambda self, x: conv(self, x))
    return seen


@pytest.mark.parametrize("kv_stride,heads", [(1, 1), (2, 2)])
def test_dec_nonlocal_output_dict_on_the_fpn_list_and_on_a_single_tensor(monkeypatch, kv_stride, heads):
    seen = _torch_ops(monkeypatch)
    torch.manual_seed(0)
    x = torch.randn(2, 32, 9, 7)
    others = [torch.randn(2, 8, 17, 13), torch.randn(2, 16, 9, 7), torch.randn(2, 24, 9, 7)]
    dec = dec_nonlocal(in_planes=32, num_classes=5, inner_planes=16, key_planes=8, value_planes=24, heads=heads, kv_stride=kv_stride,
                       scale=0.4, rep_head=True)
    a = dec(x)
    assert sorted(a) == ["pred", "rep"] and a["pred"].shape == (2, 5, 9, 7) and a["rep"].shape == (2, 256, 9, 7)
    hk, wk = (9, 7) if kv_stride == 1 else (5, 4)                             # ceil(H / 2) x ceil(W / 2)
    assert seen == [((2, 8, 9, 7), (2, 8, hk, wk), (2, 24, hk, wk), heads, 0.4)]
    # the zero-initialised norm weight makes the block the identity: the block's output is its input
    f = K.run_seq(dec.conva, x)
    assert torch.equal(dec.nl(f), f)
    with torch.no_grad():
        dec.nl.project[1].weight.fill_(0.5)
    assert not torch.equal(dec.nl(f), f)
    out = dec(others + [x])                        # the encoder's four maps: the last one is read
    assert torch.allclose(dec(x)["pred"], out["pred"])
    assert sorted(dec(others + [x], need_rep=False)) == ["pred"]
    plain = dec_nonlocal(in_planes=32, num_classes=5, inner_planes=16, key_planes=8, value_planes=8)
    assert sorted(plain(x)) == ["pred"] and sorted(plain(x, need_rep=True)) == ["pred"] and not hasattr(plain, "representation")
    assert seen[-1][3:] == (1, None)               # scale None reaches dense_attention, which takes D ** -0.5


def test_nonlocal_example_config_names_the_decoder():
    import yaml
    from u2pl_amd.models.model_helper import ModelBuilder
    with open(os.path.join(ROOT, "tools", "city_semi_nonlocal_example.yaml")) as f:
        cfg = yaml.safe_load(f)
    with open(os.path.join(ROOT, "tools", "city_semi_template.yaml")) as f:
        base = yaml.safe_load(f)
    assert cfg["net"]["decoder"] == dict(type="u2pl.models.decoder.dec_nonlocal",
                                         kwargs=dict(inner_planes=512, key_planes=64, value_planes=256, heads=1, kv_stride=1, rep_head=True))
    net = cfg["net"]
    cfg["net"]["decoder"] = base["net"]["decoder"]
    assert cfg == base                          # the template with the decoder swapped, nothing else
    with open(os.path.join(ROOT, "tools", "city_semi_nonlocal_example.yaml")) as f:
        net = yaml.safe_load(f)["net"]
    net["sync_bn"] = False
    net["encoder"]["type"] = "u2pl.models.resnet.resnet50"
    net["encoder"]["kwargs"]["pretrained"] = False
    sd = ModelBuilder(net).state_dict()
    assert "decoder.representation.4.bias" in sd and "decoder.nl.project.1.weight" in sd and "decoder.nl.value.bias" in sd


def test_half_predictor_refuses_the_decoder():
    from u2pl_amd import half
    from u2pl_amd.models.model_helper import ModelBuilder
    cfg = net_cfg("resnet50", 19, True)
    cfg["decoder"] = dict(type="u2pl.models.decoder.dec_nonlocal", kwargs=dict(rep_head=True))
    with pytest.raises(TypeError, match="decoder class dec_nonlocal is not known to the fp16 path"):
        half.HalfPredictor(ModelBuilder(cfg))
