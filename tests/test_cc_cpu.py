"""Criss-cross attention and dec_ccnet without a GPU: the float64 references of tests/cc_bounds.py are torch's float64 autograd of
the dense attention masked to the cross; the numpy fp32 emulations of the kernels' own order meet their bounds on the tables; the
named faulty emulations leave them; the calibrated ceilings are re-measured from torch's own fp32 arithmetic (-s -k ceilings
prints them); dec_ccnet builds with the documented keys, refuses what it documents and routes its inputs.  (The HIP kernels are
held to the same bounds in tests/test_gpu_cc.py.)"""
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cc_bounds as B  # noqa: E402
from model_utils import net_cfg  # noqa: E402
from u2pl_amd import nn as K  # noqa: E402
from u2pl_amd.models.decoder import dec_ccnet  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CC_HIP = open(os.path.join(ROOT, "u2pl_amd", "csrc", "ccattn.hip")).read()      # the kernels this file's emulations restate

f32, f64 = np.float32, np.float64
CPU_HW = ((1, 1), (1, 7), (7, 1), (2, 2), (3, 5), (5, 3), (9, 17), (2, 66))       # (2, 66): L = 67, a second lane register
CPU_NDC = ((1, 4, 4), (3, 20, 8))
FAULT_HW = (5, 3)                           # H != W, every pixel has row and column members, the weights are not symmetric


# ------------------------------------------------------------------ the references are torch's float64 autograd
@pytest.mark.parametrize("family", B.FAMILIES)
def test_references_are_torchs_autograd_of_the_dense_masked_attention_in_float64(family):
    for N, HW, D, C in ((1, (1, 1), 4, 4), (2, (3, 5), 4, 8), (2, (5, 3), 8, 4), (1, (1, 7), 4, 4), (1, (7, 1), 4, 4), (2, (6, 9), 20, 12)):
        q, k, v, res, g = B.cc_case(N, HW, D, C, family)
        sc, ga = B.case_scale(D), B.case_gamma(HW)
        d = B.dense64(q, k, v, res, ga, sc, g)
        r = B.cc_fwd64(q, k, v, res, ga, sc)
        assert np.abs(r["w"] - d["w"]).max() <= 1e-14 and np.abs(r["out"] - d["out"]).max() <= 1e-13 * r["unit_out"].max()
        assert np.abs(r["w"].sum(3) - 1).max() <= 1e-13                       # over the cross
        assert (r["unit_out"] >= np.abs(r["out"]) - 1e-12).all()
        b = B.cc_bwd64(g, d["w"], q, k, v, ga, sc)
        for n in B.OUTS_BWD:
            assert np.abs(b[n] - d[n]).max() <= 1e-12 * max(b["unit_" + n].max(), 1e-300), n
            assert (b["unit_" + n] >= np.abs(b[n]) - 1e-9 * b["unit_" + n].max()).all(), n
        assert np.array_equal(d["dres"], g.astype(f64))                       # the gradient of res is g itself
        # without res the output is the attention alone
        assert np.abs(B.cc_fwd64(q, k, v, None, ga, sc)["out"] - (d["out"] - res)).max() <= 1e-13 * r["unit_out"].max()


def test_the_weights_are_not_symmetric_on_the_fault_inputs():
    """w[p, m] != w[m, p]: what the gathers of dk and dv must not confuse.  (With every key the same they are all 1 / L.)"""
    H, W = FAULT_HW
    q, k, v, res, g = B.cc_case(3, FAULT_HW, 20, 8)
    w = B.cc_fwd64(q, k, v, res, 0.6, B.case_scale(20))["w"]
    assert abs(w[0, 0, 1, 0] - w[0, 0, 0, 1]) > 1e-3                          # (0, 1) -> (0, 0) against (0, 0) -> (0, 1)
    q, k, v, res, g = B.cc_case(3, FAULT_HW, 20, 8, "const")
    assert np.abs(B.cc_fwd64(q, k, v, res, 0.6, 1.0)["w"] - 1.0 / (H + W - 1)).max() <= 1e-14


def test_slot_layout_round_trip():
    for H, W in ((1, 1), (1, 4), (4, 1), (3, 5)):
        a = np.random.default_rng(H * 10 + W).standard_normal((2, H, W, H + W - 1))
        row, col = B.from_slots(a)
        assert row.shape == (2, H, W, W) and col.shape == (2, H, W, H)
        assert all(col[0, y, x, y] == 0 for y in range(H) for x in range(W))
        assert np.array_equal(B.to_slots(row, col), a)
        for y in range(H):
            for x in range(W):
                assert [a[0, y, x, W + i - (i > y)] for i in range(H) if i != y] == [col[0, y, x, i] for i in range(H) if i != y]
        rt, ct = B.from_slots(torch.from_numpy(a))
        assert np.array_equal(rt.numpy(), row) and np.array_equal(ct.numpy(), col)
        assert np.array_equal(B.to_slots(rt, ct).numpy(), a)


# ------------------------------------------------------------------ the faithful emulations inside their bounds
def emu_excess(N, HW, D, C, family, fault=None, res=True, gamma=None, scale=None):
    """-> {output: error / bound} of the emulations on one shape; fault: ("fwd" or "bwd", name) or None"""
    q, k, v, r_, g = B.cc_case(N, HW, D, C, family)
    r_ = r_ if res else None
    sc = B.case_scale(D) if scale is None else scale
    ga = B.case_gamma(HW) if gamma is None else gamma
    w, out = B.emu_fwd(q, k, v, r_, ga, sc, fault[1] if fault and fault[0] == "fwd" else None)
    e = dict(zip(("w", "out"), B.cc_fwd_excess(w, out, q, k, v, r_, ga, sc)))
    w32 = B.cc_fwd64(q, k, v, r_, ga, sc)["w"].astype(f32)
    e.update(B.cc_bwd_excess(B.emu_bwd(g, w32, q, k, v, ga, sc, fault[1] if fault and fault[0] == "bwd" else None), g, w32, q, k, v, ga, sc))
    return e


@pytest.mark.parametrize("HW", CPU_HW, ids=lambda s: "x".join(map(str, s)))
def test_emulations_of_the_kernels_order_hold_the_bounds(HW):
    for N, D, C in CPU_NDC:
        for family in B.FAMILIES:
            e = emu_excess(N, HW, D, C, family)
            assert max(e.values()) <= 1.0, (N, D, C, family, e)
    assert max(emu_excess(3, HW, 20, 8, "normal", res=False).values()) <= 1.0


def test_gamma_zero_gives_zero_gradients_but_dgamma():
    q, k, v, res, g = B.cc_case(3, (5, 3), 20, 8)
    w, out = B.emu_fwd(q, k, v, res, 0.0, 0.5)
    assert B.bits_equal(out, res)
    got = B.emu_bwd(g, w, q, k, v, 0.0, 0.5)
    assert not got["dq"].any() and not got["dk"].any() and not got["dv"].any() and abs(float(got["dgamma"][0])) > 1e-3
    assert max(B.cc_bwd_excess(got, g, w, q, k, v, 0.0, 0.5).values()) <= 1.0


def test_counts_are_the_roundings_of_the_order():
    assert [B.dot_count(c) for c in (4, 64, 260)] == [4, 64, 260]
    assert [B.lane_count(L) for L in (1, 64, 65, 128, 129, 512)] == [0, 0, 1, 1, 2, 7]
    assert [B.sum_count(P) for P in (1, 1024, 1025, 37636)] == [63, 63, 64, 99]
    assert B.bwd_counts(4, 97, 97, 512) == dict(dq=2 * 512 + 3 + 11 + 193, dk=2 * 512 + 3 + 11 + 193, dv=194, dgamma=512 + 3 + 7 + 99)


# ------------------------------------------------------------------ the calibrated ceilings, re-measured
def test_ceilings_are_what_torch_fp32_reaches():
    tor, emu = B.measure("torch"), B.measure("emu")
    print()
    for name in B.CAL:
        print(f"  CAL[{name!r:8s}] = {B.CAL[name]:<5}  torch fp32 {tor[name]:.2f}   [emulation {emu[name]:.2f}]")
    for name in B.CAL:
        assert tor[name] <= B.CAL[name] <= 2 * tor[name], (name, tor[name])
        assert emu[name] <= B.CAL_MARGIN * B.CAL[name]


# ------------------------------------------------------------------ the bounds reject faulty arithmetic
def test_fault_centre_pixel_counted_in_the_row_and_in_the_column():
    e = emu_excess(3, FAULT_HW, 20, 8, "normal", ("fwd", "centre_twice"))
    assert e["w"] > 100.0 and e["out"] > 100.0
    assert emu_excess(1, (1, 1), 4, 4, "normal", ("fwd", "centre_twice"))["w"] <= 1.0        # one pixel: its weight is 1 either way


def test_fault_row_and_column_lengths_swapped():
    e = emu_excess(3, FAULT_HW, 20, 8, "normal", ("fwd", "swapped"))
    assert e["w"] > 100.0 and e["out"] > 100.0
    assert max(emu_excess(3, (4, 4), 20, 8, "normal", ("fwd", "swapped")).values()) <= 1.0    # a square map: nothing to swap


def test_fault_no_max_subtraction_against_scores_of_100():
    assert emu_excess(1, FAULT_HW, 4, 4, "big", ("fwd", "no_max"))["w"] > 100.0               # exp(100) overflows: inf / inf
    assert emu_excess(1, FAULT_HW, 4, 4, "big")["w"] <= 1.0
    assert emu_excess(3, (2, 2), 20, 8, "const", ("fwd", "no_max"), scale=0.05)["w"] <= 1.0   # small scores: nothing to see


def test_fault_scale_dropped():
    e = emu_excess(3, FAULT_HW, 20, 8, "normal", ("fwd", "no_scale"))
    assert e["w"] > 100.0 and e["out"] > 100.0
    e = emu_excess(3, FAULT_HW, 20, 8, "normal", ("bwd", "no_scale"))
    assert e["dq"] > 100.0 and e["dk"] > 100.0 and e["dv"] <= 1.0 and e["dgamma"] <= 1.0
    assert max(emu_excess(3, FAULT_HW, 20, 8, "normal", ("bwd", "no_scale"), scale=1.0).values()) <= 1.0


def test_fault_backward_without_the_mean_term():
    e = emu_excess(3, FAULT_HW, 20, 8, "normal", ("bwd", "no_s"))
    assert e["dq"] > 100.0 and e["dk"] > 100.0 and e["dv"] <= 1.0 and e["dgamma"] <= 1.0


@pytest.mark.parametrize("out", ["dk", "dv"])
def test_fault_gather_with_the_weight_the_target_gives_to_the_source(out):
    e = emu_excess(3, FAULT_HW, 20, 8, "normal", ("bwd", out + "_wrong_w"))
    assert e[out] > 100.0 and all(val <= 1.0 for n, val in e.items() if n != out), e
    e = emu_excess(3, FAULT_HW, 20, 8, "const", ("bwd", "dv_wrong_w"))
    assert e["dv"] <= 1.0                                                      # every weight 1 / L: w[p, m] == w[m, p]
    assert emu_excess(1, (1, 1), 4, 4, "normal", ("bwd", out + "_wrong_w"))[out] <= 1.0


def test_fault_gamma_missing_from_dv_or_from_e():
    e = emu_excess(3, FAULT_HW, 20, 8, "normal", ("bwd", "dv_no_gamma"))
    assert e["dv"] > 100.0 and e["dq"] <= 1.0 and e["dk"] <= 1.0
    e = emu_excess(3, FAULT_HW, 20, 8, "normal", ("bwd", "e_no_gamma"))
    assert e["dq"] > 100.0 and e["dk"] > 100.0 and e["dv"] <= 1.0
    assert max(emu_excess(3, FAULT_HW, 20, 8, "normal", ("bwd", "e_no_gamma"), gamma=1.0).values()) <= 1.0


def test_fault_dgamma_summed_over_one_image():
    e = emu_excess(3, FAULT_HW, 20, 8, "normal", ("bwd", "dgamma_one_image"))
    assert e["dgamma"] > 100.0 and e["dq"] <= 1.0
    assert emu_excess(1, FAULT_HW, 4, 4, "normal", ("bwd", "dgamma_one_image"))["dgamma"] <= 1.0


def test_fault_names_are_the_emulations():
    assert set(B.FAULTS_FWD) == {"centre_twice", "swapped", "no_max", "no_scale"}
    assert set(B.FAULTS_BWD) == {"no_scale", "no_s", "dk_wrong_w", "dv_wrong_w", "dv_no_gamma", "e_no_gamma", "dgamma_one_image"}


# ------------------------------------------------------------------ the tables and the kernels' constants
def test_tables_use_the_constants_of_the_kernels():
    defs = {k: int(v) for k, v in re.findall(r"#define (CC_\w+) (\d+)", CC_HIP)}
    assert defs["CC_MAX_L"] == B.MAX_L == K.CC_MAX_L >= 512 and defs["CC_LCHUNK"] * defs["CC_LREGS"] == defs["CC_MAX_L"]
    assert defs["CC_LCHUNK"] == B.LCHUNK == 64 and defs["CC_LREGS"] == B.LREGS and defs["CC_PT"] == B.PT
    assert defs["CC_PASS"] == B.PASS == 256 and defs["CC_MAX_BLOCKS"] == B.GRID_CAP and defs["CC_SUM_THREADS"] == B.SUM_THREADS
    Ls = {h + w - 1 for h, w in B.CC_HW}
    assert {1, 63, 64, 65, 127, 128, 129, 255, 256, 257, B.MAX_L - 1, B.MAX_L} <= Ls and max(Ls) == B.MAX_L
    lines = {n for hw in B.CC_HW for n in hw}
    assert {B.PT - 1, B.PT + 1, 63, 64, 65, 127, 128, 129, B.MAX_L} <= lines | {7, 9}
    assert {(1, 1), (1, 7), (7, 1), (2, 2), (3, 5), (5, 3), (32, 32), (32, 33), (33, 33)} <= set(B.CC_HW)
    assert B.CC_NDC == ((1, 4, 4), (1, 260, 4), (3, 20, 64), (3, 64, 260)) and B.PASS + 4 == 260
    c = B.GRID_CASE
    H, W = c["HW"]
    waves = 4 * B.GRID_CAP
    assert c["N"] * H * W > waves and c["N"] * H * B.cdiv(W, B.PT) > waves and c["N"] * W * B.cdiv(H, B.PT) > waves
    assert c["N"] * H * W > 32 * B.SUM_THREADS
    from u2pl_amd._lib import parse_header
    decl = parse_header()
    assert [len(decl["u2pl_cc_attn_%s" % n][1]) for n in ("fwd_f32", "bwd_f32", "bwd_ws_floats")] == [20, 26, 5]
    assert decl["u2pl_cc_attn_fwd_f32"][2][8] == "gamma" and decl["u2pl_cc_attn_bwd_f32"][2][10] == "gamma"   # pointers: device memory


def test_size_query_and_refusals_need_no_gpu():
    from u2pl_amd import _lib
    L = _lib.lib()
    assert L.u2pl_cc_attn_bwd_ws_floats(4, 97, 97, 64, 512) == 4 * 9409 * 193 + 4 * 9409
    assert L.u2pl_cc_attn_bwd_ws_floats(1, 1, 1, 4, 4) == 4 + 4
    for bad in ((0, 2, 2, 4, 4), (1, 0, 2, 4, 4), (1, 2, 2, 6, 4), (1, 2, 2, 4, 0), (1, 2, B.MAX_L, 4, 4), (1, B.MAX_L + 1, 1, 4, 4)):
        assert L.u2pl_cc_attn_bwd_ws_floats(*bad) == 0
    assert L.u2pl_cc_attn_bwd_ws_floats(1, 2, B.MAX_L - 1, 4, 4) > 0
    # a refusal comes before any launch, so also without a device
    assert L.u2pl_cc_attn_fwd_f32(None, 4, None, 4, None, 4, None, 4, None, 1.0, 1, 2, 2, 4, 4, None, 3, None, 4, None) == 1001
    assert L.u2pl_cc_attn_bwd_f32(None, 4, None, 3, None, 4, None, 4, None, 4, None, 1.0, 1, 2, 2, 4, 4, None, 4, None, 4, None, 4, None,
                                  None, None) == 1001


def test_check_cc_shapes_refuses_what_the_kernels_refuse():
    assert K.check_cc_shapes(4, 97, 97, 64, 512) == (4, 97, 97, 64, 512)
    assert K.check_cc_shapes(1, 129, 257, 64, 512) == (1, 129, 257, 64, 512)              # a whole 1024 x 2048 image at stride 8
    assert K.check_cc_shapes(1, 1, K.CC_MAX_L, 4, 4) and K.check_cc_shapes(1, 256, 257, 4, 4)
    for bad in ((0, 2, 2, 4, 4), (1, 0, 2, 4, 4), (1, 2, 0, 4, 4), (1, 2, 2, 6, 4), (1, 2, 2, 4, 6), (1, 2, 2, 0, 4), (1, 2, 2, 4, 0),
                (2 ** 22, 32, 32, 4, 4)):
        with pytest.raises(ValueError):
            K.check_cc_shapes(*bad)
    with pytest.raises(ValueError, match=r"too large for one cross.*the limit is %d" % K.CC_MAX_L):
        K.check_cc_shapes(1, 257, 257, 64, 512)
    with pytest.raises(ValueError, match="too large for one cross"):
        K.check_cc_shapes(1, 1, K.CC_MAX_L + 1, 4, 4)


# ------------------------------------------------------------------ dec_ccnet
def cc_keys(in_planes=2048, num_classes=19, inner=512, key=64, recurrence=2, shared=True, rep=False):
    keys = {}

    def bn(prefix, c):
        keys.update({prefix + ".weight": (c,), prefix + ".bias": (c,), prefix + ".running_mean": (c,),
                     prefix + ".running_var": (c,), prefix + ".num_batches_tracked": ()})

    def unit3(prefix, cin, cout):
        keys[prefix + ".0.weight"] = (cout, cin, 3, 3)
        bn(prefix + ".1", cout)

    def block(prefix):
        for name, cout in (("query", key), ("key", key), ("value", inner)):
            keys.update({"%s.%s.weight" % (prefix, name): (cout, inner, 1, 1), "%s.%s.bias" % (prefix, name): (cout,)})
        keys[prefix + ".gamma"] = (1,)
    unit3("conva", in_planes, inner)
    if shared:
        block("cca")
    else:
        for i in range(recurrence):
            block("cca.%d" % i)
    unit3("convb", inner, inner)
    unit3("bottleneck", in_planes + inner, inner)
    keys.update({"classifier.weight": (num_classes, inner, 1, 1), "classifier.bias": (num_classes,)})
    if rep:
        keys["representation.0.weight"] = (256, inner, 3, 3)
        bn("representation.1", 256)
        keys.update({"representation.4.weight": (256, 256, 1, 1), "representation.4.bias": (256,)})
    return keys


@pytest.mark.parametrize("rep", [False, True])
@pytest.mark.parametrize("shared", [True, False])
def test_dec_ccnet_builds_with_the_documented_keys(shared, rep):
    dec = dec_ccnet(in_planes=2048, shared=shared, rep_head=rep)
    assert {k: tuple(v.shape) for k, v in dec.state_dict().items()} == cc_keys(shared=shared, rep=rep)
    assert isinstance(dec.bottleneck[3], torch.nn.Dropout2d) and dec.bottleneck[3].p == 0.1
    blocks = [dec.cca] if shared else list(dec.cca)
    assert len(blocks) == (1 if shared else 2) and all(float(b.gamma.detach()) == 0.0 and b.gamma.requires_grad for b in blocks)   # as in the paper
    dec = dec_ccnet(in_planes=96, num_classes=150, inner_planes=64, key_planes=8, recurrence=3, shared=shared, rep_head=rep)
    assert {k: tuple(v.shape) for k, v in dec.state_dict().items()} == cc_keys(96, 150, 64, 8, 3, shared, rep)
    if rep:
        from u2pl_amd.models.decoder import dec_pspnet
        psp = dec_pspnet(in_planes=2048, rep_head=True)
        assert [(type(a), getattr(a, "weight", torch.zeros(0)).shape) for a in dec_ccnet(2048, rep_head=True).representation] == \
            [(type(a), getattr(a, "weight", torch.zeros(0)).shape) for a in psp.representation]


def test_dec_ccnet_refuses_what_it_documents():
    for kw in (dict(in_planes=2046), dict(in_planes=2048, inner_planes=510), dict(in_planes=2048, key_planes=30),
               dict(in_planes=2048, key_planes=0)):
        with pytest.raises(ValueError, match="multiple of 4"):
            dec_ccnet(**kw)
    with pytest.raises(ValueError, match="recurrence"):
        dec_ccnet(in_planes=2048, recurrence=0)
    for nc in (0, 1, 256):
        with pytest.raises(ValueError, match="num_classes"):
            dec_ccnet(in_planes=2048, num_classes=nc)
    with pytest.raises(TypeError):
        dec_ccnet(in_planes=2048, heads=2)           # no multi-head form
    with pytest.raises(TypeError):
        dec_ccnet(in_planes=2048, separable=True)    # no separable form
    dec_ccnet(in_planes=48, num_classes=255, inner_planes=8, key_planes=4, recurrence=1)


def test_dec_ccnet_resolves_through_the_alias_package_and_model_builder():
    import importlib
    from u2pl_amd.models.model_helper import ModelBuilder
    assert importlib.import_module("u2pl.models.decoder").dec_ccnet is dec_ccnet
    cfg = net_cfg("resnet50", 19, True)
    cfg["decoder"] = dict(type="u2pl.models.decoder.dec_ccnet", kwargs=dict(rep_head=True, shared=False))
    model = ModelBuilder(cfg)
    assert isinstance(model.decoder, dec_ccnet) and model.decoder.recurrence == 2
    sd = model.state_dict()
    assert tuple(sd["decoder.conva.0.weight"].shape) == (512, 2048, 3, 3)
    assert tuple(sd["decoder.cca.1.key.weight"].shape) == (64, 512, 1, 1) and tuple(sd["decoder.cca.0.gamma"].shape) == (1,)
    assert tuple(sd["decoder.bottleneck.0.weight"].shape) == (512, 2560, 3, 3)
    assert tuple(sd["decoder.representation.4.weight"].shape) == (256, 256, 1, 1)
    assert tuple(sd["auxor.aux.0.weight"].shape) == (256, 1024, 3, 3)


def _torch_ops(monkeypatch):
    """the decoder's wiring without a GPU: every u2pl_amd.nn operation it calls replaced by the torch function it stands for, and
    the attention calls recorded (the HIP operations themselves are tests/test_gpu_cc.py's)"""
    seen = []

    def seq(s, x):
        for m in s:
            if isinstance(m, K.Conv2d):
                x = F.conv2d(x, m.weight, m.bias, padding=m.padding)
            elif isinstance(m, K.BatchNorm2d):
                x = F.batch_norm(x, None, None, m.weight, m.bias, training=True)
            elif isinstance(m, torch.nn.ReLU):
                x = torch.relu(x)
        return x

    def attention(q, k, v, gamma, res=None, scale=1.0):
        seen.append((tuple(q.shape), tuple(k.shape), tuple(v.shape), gamma, res, scale))
        perm = [t.permute(0, 2, 3, 1) for t in (q, k, v)]
        y = B.mix(torch.softmax(B.dots(perm[0], perm[1]) * scale, 3), perm[2]).permute(0, 3, 1, 2)
        return res + gamma * y

    monkeypatch.setattr(K, "criss_cross_attention", attention)
    monkeypatch.setattr(K, "cat_channels", lambda ts: torch.cat(tuple(ts), 1))
    monkeypatch.setattr(K, "run_seq", lambda s, x, grad_link=None: seq(s, x))
    monkeypatch.setattr(K.Conv2d, "forward", lambda self, x: F.conv2d(x, self.weight, self.bias, padding=self.padding))
    return seen


@pytest.mark.parametrize("shared", [True, False])
def test_dec_ccnet_output_dict_on_the_fpn_list_and_on_a_single_tensor(monkeypatch, shared):
    seen = _torch_ops(monkeypatch)
    torch.manual_seed(0)
    x = torch.randn(2, 32, 9, 7)
    others = [torch.randn(2, 8, 17, 13), torch.randn(2, 16, 9, 7), torch.randn(2, 24, 9, 7)]
    dec = dec_ccnet(in_planes=32, num_classes=5, inner_planes=16, key_planes=8, recurrence=3, shared=shared, rep_head=True)
    blocks = [dec.cca] * 3 if shared else list(dec.cca)
    with torch.no_grad():
        for i, b in enumerate(blocks):
            b.gamma.fill_(0.5 + i)
    a = dec(x)
    assert sorted(a) == ["pred", "rep"] and a["pred"].shape == (2, 5, 9, 7) and a["rep"].shape == (2, 256, 9, 7)
    assert len(seen) == 3                          # `recurrence` rounds, each on the round before
    for (qs, ks, vs, gamma, res, scale), b in zip(seen, blocks):
        assert (qs, ks, vs) == ((2, 8, 9, 7), (2, 8, 9, 7), (2, 16, 9, 7)) and gamma is b.gamma and scale == 1.0
        assert tuple(res.shape) == (2, 16, 9, 7)
    assert not torch.equal(seen[0][4], seen[1][4]) and not torch.equal(seen[1][4], seen[2][4])
    out = dec(others + [x])                        # the encoder's four maps: the last one is read
    assert all(torch.equal(a[k], out[k]) for k in a)
    assert sorted(dec(others + [x], need_rep=False)) == ["pred"]
    plain = dec_ccnet(in_planes=32, num_classes=5, inner_planes=16, key_planes=8, shared=shared)
    assert sorted(plain(x)) == ["pred"] and sorted(plain(x, need_rep=True)) == ["pred"] and not hasattr(plain, "representation")


def test_ccnet_example_config_names_the_decoder():
    import yaml
    from u2pl_amd.models.model_helper import ModelBuilder
    with open(os.path.join(ROOT, "tools", "city_semi_ccnet_example.yaml")) as f:
        cfg = yaml.safe_load(f)
    with open(os.path.join(ROOT, "tools", "city_semi_template.yaml")) as f:
        base = yaml.safe_load(f)
    assert cfg["net"]["decoder"] == dict(type="u2pl.models.decoder.dec_ccnet",
                                         kwargs=dict(inner_planes=512, key_planes=64, recurrence=2, shared=True, rep_head=True))
    cfg["net"]["decoder"] = base["net"]["decoder"]
    assert cfg == base                          # the template with the decoder swapped, nothing else
    with open(os.path.join(ROOT, "tools", "city_semi_ccnet_example.yaml")) as f:
        net = yaml.safe_load(f)["net"]
    net["sync_bn"] = False
    net["encoder"]["type"] = "u2pl.models.resnet.resnet50"
    net["encoder"]["kwargs"]["pretrained"] = False
    sd = ModelBuilder(net).state_dict()
    assert "decoder.representation.4.bias" in sd and "decoder.cca.gamma" in sd and "decoder.cca.value.bias" in sd


def test_half_predictor_refuses_the_decoder():
    from u2pl_amd import half
    from u2pl_amd.models.model_helper import ModelBuilder
    cfg = net_cfg("resnet50", 19, True)
    cfg["decoder"] = dict(type="u2pl.models.decoder.dec_ccnet", kwargs=dict(rep_head=True))
    with pytest.raises(TypeError, match="decoder class dec_ccnet is not known to the fp16 path"):
        half.HalfPredictor(ModelBuilder(cfg))


def test_shared_weights_are_refused_under_a_process_group(monkeypatch):
    """with shared weights every round adds into the same gradient sinks, and the bucketed all-reduce counts one arrival per
    parameter: refused by name where the step learns that it runs on more than one rank (or under U2PL_DIST_SINGLE)"""
    seen = _torch_ops(monkeypatch)
    x = torch.randn(2, 32, 5, 4)
    monkeypatch.setattr(K, "dist_active", lambda: True)
    dec = dec_ccnet(in_planes=32, num_classes=5, inner_planes=16, key_planes=8)
    with pytest.raises(NotImplementedError, match=r"shared attention weights.*more than one rank or under U2PL_DIST_SINGLE.*"
                                                  r"`shared: false` or `recurrence: 1` run there"):
        dec(x)
    assert not seen
    with torch.no_grad():
        assert sorted(dec(x)) == ["pred"]          # nothing is reduced without a gradient: the teacher's and eval's passes run
    for kw in (dict(shared=False), dict(recurrence=1)):
        assert sorted(dec_ccnet(in_planes=32, num_classes=5, inner_planes=16, key_planes=8, **kw)(x)) == ["pred"]
    monkeypatch.setattr(K, "dist_active", lambda: False)
    assert sorted(dec(x)) == ["pred"]
