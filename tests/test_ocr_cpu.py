"""Region pool, region attention and dec_ocrnet without a GPU: the float64 references of tests/ocr_bounds.py are torch's float64
autograd of the plain formulas; the numpy fp32 emulations of the kernels' own order meet their bounds on the tables; the named
faulty emulations leave them; the calibrated ceilings are re-measured from torch's own fp32 arithmetic (-s -k ceilings prints
them); dec_ocrnet builds with the documented keys, refuses what the kernels refuse and routes its inputs; the trainer adds the
region term only for outputs that carry it.  (The HIP kernels are held to the same bounds in tests/test_gpu_ocr.py.)"""
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ocr_bounds as B  # noqa: E402
from model_utils import net_cfg  # noqa: E402
from u2pl_amd import nn as K  # noqa: E402
from u2pl_amd.models.decoder import dec_ocrnet  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OCR_HIP = open(os.path.join(ROOT, "u2pl_amd", "csrc", "ocr.hip")).read()      # the kernels this file's emulations restate

f32, f64 = np.float32, np.float64
T = torch.from_numpy
CPU_C = (4, 20)         # the emulations are loops over pixels and regions: the channel edges (C = 260) are the GPU file's
CPU_K = (1, 2, 19, B.KT + 1, B.KCHUNK + 1)


# ------------------------------------------------------------------ the references are torch's float64 autograd
@pytest.mark.parametrize("family", B.FAMILIES)
def test_region_pool_references_are_torchs_autograd_in_float64(family):
    for N, hw, Kr, C in ((1, 1, 1, 4), (3, 6, 2, 4), (2, 70, 19, 8), (2, 300, 5, 4)):
        s, x, g, add = B.pool_case(N, hw, Kr, C, family)
        sc = B.pool_scale(N)
        st, xt = T(s.astype(f64)).requires_grad_(True), T(x.astype(f64)).requires_grad_(True)
        m = torch.softmax(float(f32(sc)) * st, 1)
        f = m.transpose(1, 2) @ xt
        ((f * T(g.astype(f64))).sum() + (xt * T(add.astype(f64))).sum()).backward()
        r = B.pool_fwd64(s, x, sc)
        assert np.abs(r["m"] - m.detach().numpy()).max() <= 1e-14 and np.abs(r["f"] - f.detach().numpy()).max() <= 1e-13 * r["unit_f"].max()
        b = B.pool_bwd64(g, r["m"], x, r["f"], add, sc)
        assert np.abs(b["dx"] - xt.grad.numpy()).max() <= 1e-13 * b["unit_dx"].max()
        assert np.abs(b["ds"] - st.grad.numpy()).max() <= 1e-13 * max(b["unit_ds"].max(), 1e-300)
        assert (b["unit_dx"] >= np.abs(b["dx"]) - 1e-12).all() and (b["unit_ds"] >= np.abs(b["ds"]) - 1e-12).all()
        assert np.abs(r["m"].sum(1) - 1).max() <= 1e-13                      # over the pixels of an image


@pytest.mark.parametrize("family", B.FAMILIES)
def test_region_attention_references_are_torchs_autograd_in_float64(family):
    for N, hw, Kr, Dm in ((1, 1, 1, 4), (3, 6, 2, 4), (2, 70, 19, 8), (2, 9, 70, 20)):
        q, kk, v, gy = B.attn_case(N, hw, Kr, Dm, family)
        sc = B.attn_scale(Dm)
        qt, kt, vt = (T(t.astype(f64)).requires_grad_(True) for t in (q, kk, v))
        w = torch.softmax(float(f32(sc)) * (qt @ kt.transpose(1, 2)), 2)
        y = w @ vt
        (y * T(gy.astype(f64))).sum().backward()
        r = B.attn_fwd64(q, kk, v, sc)
        assert np.abs(r["w"] - w.detach().numpy()).max() <= 1e-14 and np.abs(r["y"] - y.detach().numpy()).max() <= 1e-13 * r["unit_y"].max()
        b = B.attn_bwd64(gy, r["w"], q, kk, v, sc)
        for k, t in (("dq", qt), ("dk", kt), ("dv", vt)):
            assert np.abs(b[k] - t.grad.numpy()).max() <= 1e-12 * max(b["unit_" + k].max(), 1e-300), k
            assert (b["unit_" + k] >= np.abs(b[k]) - 1e-9 * b["unit_" + k].max()).all()
        assert np.abs(r["w"].sum(2) - 1).max() <= 1e-13                      # over the regions


# ------------------------------------------------------------------ the faithful emulations inside their bounds
def emu_excess(N, hw, Kr, C, family, fault=None):
    """-> {output: error / bound} of the emulations on one shape; fault: (entry point, name) or None"""
    fp = {k: (fault[1] if fault and fault[0] == k else None) for k in ("pool_fwd", "pool_bwd", "attn_fwd", "attn_bwd")}
    s, x, g, add = B.pool_case(N, hw, Kr, C, family)
    sc = B.pool_scale(N)
    m, f = B.emu_pool_fwd(s, x, sc, fp["pool_fwd"])
    out = dict(zip(("m", "f"), B.pool_fwd_excess(m, f, s, x, sc)))
    r = B.pool_fwd64(s, x, sc)
    m32, f32_ = r["m"].astype(f32), r["f"].astype(f32)
    dx, ds = B.emu_pool_bwd(g, m32, x, f32_, add, sc, fp["pool_bwd"])
    out.update(zip(("dx", "ds"), B.pool_bwd_excess(dx, ds, g, m32, x, f32_, add, sc)))
    q, kk, v, gy = B.attn_case(N, hw, Kr, C, family)
    sc = B.attn_scale(C)
    w, y = B.emu_attn_fwd(q, kk, v, sc, fp["attn_fwd"])
    out.update(zip(("w", "y"), B.attn_fwd_excess(w, y, q, kk, v, sc)))
    w32 = B.attn_fwd64(q, kk, v, sc)["w"].astype(f32)
    out.update(B.attn_bwd_excess(B.emu_attn_bwd(gy, w32, q, kk, v, sc, fp["attn_bwd"]), gy, w32, q, kk, v, sc))
    return out


@pytest.mark.parametrize("Kr", CPU_K)
@pytest.mark.parametrize("HW", B.OCR_HW, ids=lambda s: "x".join(map(str, s)))
def test_emulations_of_the_kernels_order_hold_the_bounds(HW, Kr):
    for N, C in zip(B.OCR_N, CPU_C):
        for family in B.FAMILIES if B.hw_of(HW) <= 70 else ("normal",):
            e = emu_excess(N, B.hw_of(HW), Kr, C, family)
            assert max(e.values()) <= 1.0, (N, C, family, e)


def test_emulations_hold_the_bounds_without_add_and_without_a_gradient():
    s, x, g, add = B.pool_case(3, 70, 19, 20)
    r = B.pool_fwd64(s, x, 0.7)
    m32, f32_ = r["m"].astype(f32), r["f"].astype(f32)
    for g_, a_ in ((g, None), (None, add), (None, None)):
        dx, ds = B.emu_pool_bwd(g_, m32, x, f32_, a_, 0.7)
        assert max(B.pool_bwd_excess(dx, ds, g_, m32, x, f32_, a_, 0.7)) <= 1.0
        if g_ is None:
            assert not ds.any() and (B.bits_equal(dx, add) if a_ is not None else not dx.any())


def test_counts_are_the_roundings_of_the_order():
    assert [B.dot_count(c) for c in (4, 256, 260, 512)] == [11, 11, 12, 12]
    assert [B.col_count(hw, 19) for hw in (1, 13, 14, 256, 257)] == [0, 12, 13, 19 + 12, 19 + 12 + 1]    # R = 13 rows
    assert [B.col_count(hw, 255) for hw in (1, 256, 513)] == [0, 255, 257]                              # R = 1: one chain
    assert [B.wsum_count(hw) for hw in (1, 64, 65, 256, 257, 9409)] == [1, 64, 65, 67, 68, 103]


# ------------------------------------------------------------------ the calibrated ceilings, re-measured
def test_ceilings_are_what_torch_fp32_reaches():
    tor, emu = B.measure("torch"), B.measure("emu")
    print()
    for name in B.CAL:
        print(f"  CAL[{name!r:4s}] = {B.CAL[name]:<5}  torch fp32 {tor[name]:.2f}   [emulation {emu[name]:.2f}]")
    for name in B.CAL:
        assert tor[name] <= B.CAL[name] <= 2 * tor[name], (name, tor[name])
        assert emu[name] <= B.CAL_MARGIN * B.CAL[name]


# ------------------------------------------------------------------ the bounds reject faulty arithmetic
def test_fault_no_max_subtraction_against_logits_of_100():
    for what, out in (("pool_fwd", "m"), ("attn_fwd", "w")):
        assert emu_excess(1, 70, 19, 4, "big", (what, "no_max"))[out] > 100.0           # exp(100) overflows: inf / inf
        assert emu_excess(1, 70, 19, 4, "big")[out] <= 1.0                              # (N = 1: the pool's scale is 1.0)
        assert emu_excess(3, 6, 2, 20, "normal", (what, "no_max"))[out] <= 1.0          # small logits: nothing to see


def test_fault_region_softmax_over_the_classes_of_a_pixel():
    e = emu_excess(3, 70, 19, 20, "normal", ("pool_fwd", "over_classes"))
    assert e["m"] > 100.0 and e["f"] > 100.0
    assert emu_excess(1, 1, 1, 4, "normal", ("pool_fwd", "over_classes"))["m"] <= 1.0     # one pixel, one class: both are 1


def test_fault_region_softmax_over_the_whole_batch():
    e = emu_excess(3, 70, 19, 20, "normal", ("pool_fwd", "whole_batch"))
    assert e["m"] > 100.0 and e["f"] > 100.0
    assert emu_excess(1, 70, 19, 4, "normal", ("pool_fwd", "whole_batch"))["m"] <= 1.0    # one image: the batch is the image


def test_fault_attention_scale_dropped():
    e = emu_excess(3, 70, 19, 20, "normal", ("attn_fwd", "no_scale"))
    assert e["w"] > 100.0 and e["y"] > 100.0
    assert emu_excess(3, 70, 1, 20, "normal", ("attn_fwd", "no_scale"))["w"] <= 1.0       # one region: the weight is 1


def test_fault_backward_without_the_mean_term():
    assert emu_excess(3, 70, 19, 20, "normal", ("pool_bwd", "no_c"))["ds"] > 100.0
    e = emu_excess(3, 70, 19, 20, "normal", ("attn_bwd", "no_sd"))
    assert e["dq"] > 100.0 and e["dk"] > 100.0 and e["dv"] <= 1.0


def test_fault_dk_without_scale():
    e = emu_excess(3, 70, 19, 20, "normal", ("attn_bwd", "dk_no_scale"))
    assert e["dk"] > 100.0 and e["dq"] <= 1.0 and e["dv"] <= 1.0
    assert emu_excess(1, 70, 19, 4, "normal", ("attn_bwd", "dk_no_scale"))["dk"] > 100.0  # (scale = 0.5)


def test_tables_use_the_constants_of_the_kernels():
    defs = {k: int(v) for k, v in re.findall(r"#define (OCR_\w+) (\d+)", OCR_HIP)}
    assert defs["OCR_SLAB"] == B.SLAB and defs["OCR_WAVE_PX"] == B.WAVE_PX == B.SLAB // 4 and defs["OCR_KT"] == B.KT
    assert defs["OCR_KCHUNK"] == B.KCHUNK and defs["OCR_KCHUNK"] * defs["OCR_KREGS"] > defs["OCR_MAX_K"] == B.MAX_K == K.REGION_MAX_K
    assert defs["OCR_PX"] == B.PX and defs["OCR_PASS"] == B.PASS and defs["OCR_MAX_BLOCKS"] == B.GRID_CAP
    assert {B.KT - 1, B.KT, B.KT + 1, B.KCHUNK - 1, B.KCHUNK, B.KCHUNK + 1, 1, 2, 19, 33, 255} == set(B.OCR_K)
    assert B.PASS + 4 in B.OCR_C and (1, B.SLAB + 1) in B.OCR_HW
    c = B.GRID_CASE
    hw = B.hw_of(c["HW"])
    assert B.GRID_CAP < c["N"] * B.cdiv(hw, B.SLAB) <= B.GRID_CAP + 3 and c["N"] * B.cdiv(hw, B.PX) > 4 * B.GRID_CAP
    c = B.REDUCE_GRID_CASE
    assert 256 * B.GRID_CAP < c["N"] * c["K"] * c["C"] // 4 <= 256 * B.GRID_CAP + 3 * c["K"] * 4 and c["K"] == B.MAX_K
    c = B.ROWDOT_GRID_CASE
    assert 4 * B.GRID_CAP < c["N"] * c["K"] <= 4 * B.GRID_CAP + c["K"] and c["K"] == B.MAX_K
    from u2pl_amd._lib import parse_header
    decl = parse_header()
    assert [len(decl["u2pl_region_%s_f32" % n][1]) for n in ("pool_fwd", "pool_bwd", "attn_fwd", "attn_bwd")] == [15, 21, 16, 23]
    assert all(len(decl["u2pl_region_%s_ws_floats" % n][1]) == 4 for n in ("pool_fwd", "pool_bwd", "attn_bwd"))


def test_check_region_shapes_refuses_what_the_kernels_refuse():
    assert K.check_region_shapes(4, 97 * 97, 19, 512) == (4, 9409, 19, 512)
    for bad in ((1, 4, 0, 8), (1, 4, 256, 8), (1, 4, 2, 6), (1, 4, 2, 0), (0, 4, 2, 8), (1, 0, 2, 8), (2, 2 ** 30, 2, 8)):
        with pytest.raises(ValueError):
            K.check_region_shapes(*bad)


# ------------------------------------------------------------------ dec_ocrnet
def ocr_keys(in_planes=2048, num_classes=19, inner=512, key=256, rep=False):
    keys = {}

    def bn(prefix, c):
        keys.update({prefix + ".weight": (c,), prefix + ".bias": (c,), prefix + ".running_mean": (c,),
                     prefix + ".running_var": (c,), prefix + ".num_batches_tracked": ()})

    def unit(prefix, i, cin, cout):
        keys["%s.%d.weight" % (prefix, i)] = (cout, cin, 1, 1)
        bn("%s.%d" % (prefix, i + 1), cout)
    keys["conv3x3.0.weight"] = (inner, in_planes, 3, 3)
    bn("conv3x3.1", inner)
    unit("region", 0, in_planes, 256)
    keys.update({"region.3.weight": (num_classes, 256, 1, 1), "region.3.bias": (num_classes,)})
    for name in ("f_pixel", "f_object"):
        unit(name, 0, inner, key)
        unit(name, 3, key, key)
    unit("f_down", 0, inner, key)
    unit("f_up", 0, key, inner)
    unit("fuse", 0, 2 * inner, inner)
    keys.update({"classifier.weight": (num_classes, inner, 1, 1), "classifier.bias": (num_classes,)})
    if rep:
        keys["representation.0.weight"] = (256, inner, 3, 3)
        bn("representation.1", 256)
        keys.update({"representation.4.weight": (256, 256, 1, 1), "representation.4.bias": (256,)})
    return keys


@pytest.mark.parametrize("rep", [False, True])
def test_dec_ocrnet_builds_with_the_documented_keys(rep):
    dec = dec_ocrnet(in_planes=2048, rep_head=rep)
    assert {k: tuple(v.shape) for k, v in dec.state_dict().items()} == ocr_keys(rep=rep)
    assert isinstance(dec.fuse[3], torch.nn.Dropout2d) and dec.fuse[3].p == 0.05 and dec.region_loss_weight == 0.4
    dec = dec_ocrnet(in_planes=96, num_classes=150, inner_planes=64, key_planes=32, rep_head=rep, region_loss_weight=0)
    assert {k: tuple(v.shape) for k, v in dec.state_dict().items()} == ocr_keys(96, 150, 64, 32, rep)
    if rep:
        from u2pl_amd.models.decoder import dec_pspnet
        psp = dec_pspnet(in_planes=2048, rep_head=True)
        assert [(type(a), getattr(a, "weight", torch.zeros(0)).shape) for a in dec_ocrnet(2048, rep_head=True).representation] == \
            [(type(a), getattr(a, "weight", torch.zeros(0)).shape) for a in psp.representation]


def test_dec_ocrnet_refuses_what_the_kernels_refuse():
    with pytest.raises(ValueError, match="regions <= 255"):
        dec_ocrnet(in_planes=2048, num_classes=256)
    with pytest.raises(ValueError, match="regions <= 255"):
        dec_ocrnet(in_planes=2048, num_classes=0)
    with pytest.raises(ValueError, match="multiple of 4"):
        dec_ocrnet(in_planes=2048, inner_planes=510)
    with pytest.raises(ValueError, match="multiple of 4"):
        dec_ocrnet(in_planes=2048, key_planes=30)
    with pytest.raises(ValueError, match="multiple of 4"):
        dec_ocrnet(in_planes=2046)
    with pytest.raises(ValueError, match="region_loss_weight"):
        dec_ocrnet(in_planes=2048, region_loss_weight=-0.1)
    with pytest.raises(TypeError):
        dec_ocrnet(in_planes=2048, heads=2)           # no multi-head form
    with pytest.raises(TypeError):
        dec_ocrnet(in_planes=2048, separable=True)    # no separable form
    dec_ocrnet(in_planes=48, num_classes=255, inner_planes=8, key_planes=4)


def test_dec_ocrnet_resolves_through_the_alias_package_and_model_builder():
    import importlib
    from u2pl_amd.models.model_helper import ModelBuilder
    assert importlib.import_module("u2pl.models.decoder").dec_ocrnet is dec_ocrnet
    cfg = net_cfg("resnet50", 19, True)
    cfg["decoder"] = dict(type="u2pl.models.decoder.dec_ocrnet", kwargs=dict(rep_head=True))
    model = ModelBuilder(cfg)
    assert isinstance(model.decoder, dec_ocrnet) and model.decoder.key_planes == 256
    sd = model.state_dict()
    assert tuple(sd["decoder.conv3x3.0.weight"].shape) == (512, 2048, 3, 3)
    assert tuple(sd["decoder.region.3.weight"].shape) == (19, 256, 1, 1)
    assert tuple(sd["decoder.representation.4.weight"].shape) == (256, 256, 1, 1)
    assert tuple(sd["auxor.aux.0.weight"].shape) == (256, 1024, 3, 3)


def _torch_ops(monkeypatch):
    """the decoder's wiring without a GPU: every u2pl_amd.nn operation it calls replaced by the torch function it stands for, and
    the calls recorded (the HIP operations themselves are tests/test_gpu_ocr.py's)"""
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

    def unit(c, b, x):
        return torch.relu(F.batch_norm(F.conv2d(x, c.weight), None, None, b.weight, b.bias, training=True))

    def region_pool(x, s, scale=1.0):
        seen.append(("region_pool", tuple(x.shape), tuple(s.shape), scale))
        m = torch.softmax(scale * s.flatten(2), 2)
        return x, torch.einsum("nkp,ncp->nck", m, x.flatten(2)).unsqueeze(3)

    def region_attention(q, kk, v, scale):
        seen.append(("region_attention", tuple(q.shape), tuple(kk.shape), tuple(v.shape), scale))
        w = torch.softmax(scale * torch.einsum("ndp,ndk->npk", q.flatten(2), kk.squeeze(3)), 2)
        return torch.einsum("npk,ndk->ndp", w, v.squeeze(3)).reshape(q.shape)

    def group(units):
        seen.append(("conv_bn_group", len(units), [u[0] for u in units]))
        return [unit(c, b, x) for c, b, x, r, d in units]
    monkeypatch.setattr(K, "region_pool", region_pool)
    monkeypatch.setattr(K, "region_attention", region_attention)
    monkeypatch.setattr(K, "conv_bn_group", group)
    monkeypatch.setattr(K, "conv_bn", lambda c, b, x, relu=False: unit(c, b, x))
    monkeypatch.setattr(K, "cat_channels", lambda ts: torch.cat(tuple(ts), 1))
    monkeypatch.setattr(K, "run_seq", lambda s, x, grad_link=None: seq(s, x))
    monkeypatch.setattr(K.Conv2d, "forward", lambda self, x: F.conv2d(x, self.weight, self.bias, padding=self.padding))
    return seen


def test_dec_ocrnet_output_dict_on_the_fpn_list_and_on_a_single_tensor(monkeypatch):
    seen = _torch_ops(monkeypatch)
    torch.manual_seed(0)
    x = torch.randn(2, 32, 9, 7)
    others = [torch.randn(2, 8, 17, 13), torch.randn(2, 16, 9, 7), torch.randn(2, 24, 9, 7)]
    dec = dec_ocrnet(in_planes=32, num_classes=5, inner_planes=16, key_planes=8, rep_head=True)
    a = dec(x)
    assert sorted(a) == ["pred", "region", "rep"]
    assert a["pred"].shape == (2, 5, 9, 7) and a["region"].shape == (2, 5, 9, 7) and a["rep"].shape == (2, 256, 9, 7)
    assert seen[0] == ("region_pool", (2, 16, 9, 7), (2, 5, 9, 7), 1.0)
    assert seen[1][:2] == ("conv_bn_group", 2) and seen[1][2] == [dec.f_object[0], dec.f_down[0]]
    assert seen[2] == ("region_attention", (2, 8, 9, 7), (2, 8, 5, 1), (2, 8, 5, 1), 8 ** -0.5)
    b = dec(others + [x])                       # the encoder's four maps: the last one is read
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert sorted(dec(others + [x], need_rep=False)) == ["pred", "region"]
    plain = dec_ocrnet(in_planes=32, num_classes=5, inner_planes=16, key_planes=8)
    assert sorted(plain(x)) == ["pred", "region"] and sorted(plain(x, need_rep=True)) == ["pred", "region"]
    assert not hasattr(plain, "representation")


def test_ocrnet_example_config_names_the_decoder():
    import yaml
    from u2pl_amd.models.model_helper import ModelBuilder
    with open(os.path.join(ROOT, "tools", "city_semi_ocrnet_example.yaml")) as f:
        cfg = yaml.safe_load(f)
    with open(os.path.join(ROOT, "tools", "city_semi_template.yaml")) as f:
        base = yaml.safe_load(f)
    assert cfg["net"]["decoder"] == dict(type="u2pl.models.decoder.dec_ocrnet",
                                         kwargs=dict(inner_planes=512, key_planes=256, rep_head=True, region_loss_weight=0.4))
    cfg["net"]["decoder"] = base["net"]["decoder"]
    assert cfg == base                          # the template with the decoder swapped, nothing else
    with open(os.path.join(ROOT, "tools", "city_semi_ocrnet_example.yaml")) as f:
        net = yaml.safe_load(f)["net"]
    net["sync_bn"] = False
    net["encoder"]["type"] = "u2pl.models.resnet.resnet50"
    net["encoder"]["kwargs"]["pretrained"] = False
    sd = ModelBuilder(net).state_dict()
    assert "decoder.representation.4.bias" in sd and "decoder.region.3.bias" in sd


def test_half_predictor_refuses_the_decoder():
    from u2pl_amd import half
    from u2pl_amd.models.model_helper import ModelBuilder
    cfg = net_cfg("resnet50", 19, True)
    cfg["decoder"] = dict(type="u2pl.models.decoder.dec_ocrnet", kwargs=dict(rep_head=True))
    with pytest.raises(TypeError, match="decoder class dec_ocrnet is not known to the fp16 path"):
        half.HalfPredictor(ModelBuilder(cfg))


# ------------------------------------------------------------------ the trainer adds the region term only where it is asked for
class _Stub:
    def __init__(self, weight=None):
        self.decoder = type("D", (), {})()
        if weight is not None:
            self.decoder.region_loss_weight = weight


def test_trainer_adds_the_region_term_only_when_the_key_is_present(monkeypatch):
    from u2pl_amd import trainer as TR
    calls = []
    monkeypatch.setattr(TR.H, "bilinear_up", lambda x, size: calls.append(("up", tuple(x.shape), tuple(size))) or x)
    monkeypatch.setattr(TR.H, "cross_entropy",
                        lambda logits, target, ignore_index=255, **kw: calls.append(("ce", tuple(logits.shape), ignore_index, kw))
                        or torch.tensor(2.0))
    cfg = dict(dataset=dict(ignore_label=254))
    sup, label = torch.tensor(1.0), torch.zeros(2, 8, 8, dtype=torch.long)
    outs = dict(pred=torch.zeros(4, 19, 3, 3), rep=torch.zeros(4, 256, 3, 3))
    for model in (_Stub(), _Stub(0.4), object()):
        assert TR.add_region_loss(sup, model, outs, 2, (8, 8), label, cfg) is sup      # no "region": nothing is called
    outs["region"] = torch.zeros(4, 19, 3, 3)
    for model in (_Stub(), _Stub(0.0), object()):
        assert TR.add_region_loss(sup, model, outs, 2, (8, 8), label, cfg) is sup      # no weight: nothing is called
    assert not calls
    got = TR.add_region_loss(sup, _Stub(0.4), outs, 2, (8, 8), label, cfg)
    assert float(got) == 3.0
    assert calls == [("up", (2, 19, 3, 3), (8, 8)), ("ce", (2, 19, 3, 3), 254, dict(scale=0.4))]      # the labelled half, plain CE
