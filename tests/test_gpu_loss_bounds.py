"""The per-pixel loss heads against float64 at every class count and edge: cross entropy forward and backward (plain, unsup
weight, class weights), the OHEM probability and kept-target rewrite, pseudo label, entropy (stand-alone and every fused
up-sampling route), the confusion histogram and the bilinear backward, each inside the bound of tests/loss_bounds.py (derived count
and the bound calibrated from the reference's own fp32 arithmetic, the smaller) on EVERY element, the integer outputs exactly,
and once more at the first sizes that take a second grid-stride trip.  The references are loss_bounds' float64 ones, evaluated
on the device of their fp32 inputs; tests/test_loss_bounds_cpu.py pins them and shows that the bounds reject faulty arithmetic."""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_bounds as LB  # noqa: E402
from oracle import restate as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
IGN = LB.IGNORE
CS = [(C, s) for C in LB.CLASSES for s in LB.SHAPES]
CS_IDS = [f"C{C}-{'x'.join(map(str, s))}" for C, s in CS]
# (unsup_weight, class weights, scale, upstream gradient): scale in {1.0, 0.4}, an upstream gradient that is not 1, of either sign
CE_FORMS = (("plain", False, False, 1.0, 1.0), ("unsup", True, False, 0.4, 1.7), ("weighted", False, True, 0.4, -0.6))


def hip():
    from u2pl_amd import hipops as H
    return H


def call(*a):
    from u2pl_amd._lib import call as c
    return c(*a)


def D(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t.to(dtype) if dtype is not None else t


@functools.lru_cache(maxsize=None)
def case(family, C, shape):
    """logits, targets and the float64 softmax of a family, made once and shared (never modified)"""
    z, tgt = LB.make_case(family, C, shape)
    zd = D(z)
    return dict(z=z, tgt=tgt, zd=zd, sm=LB.softmax64(zd), zmax=float(np.abs(z).max()), argmax=z.argmax(1))


@functools.lru_cache(maxsize=None)
def target(family, C, shape, pat):
    t = LB.apply_ignore(case(family, C, shape)["tgt"], pat)
    return t, D(t)


def device_ce(zd, td, unsup, cw, gmul, gout):
    """loss and gradient through hipops.cross_entropy, out3 through the C ABI (the wrapper keeps it to itself)"""
    H = hip()
    x = zd.detach().requires_grad_(True)
    loss = H.cross_entropy(x, td, IGN, unsup_weight=unsup, scale=gmul, class_weight=cw)
    loss.backward(torch.tensor(gout, dtype=torch.float32, device=DEV))
    N, C, Hh, W = zd.shape
    from u2pl_amd._lib import query
    work = torch.empty(query("u2pl_ce_workspace_bytes"), dtype=torch.uint8, device=DEV)
    out3 = torch.full((3,), -7.0, dtype=torch.float32, device=DEV)
    xc = zd.contiguous()
    if cw is not None:
        call("u2pl_ce_fwd_weighted_f32", xc, td, IGN, N, C, Hh, W, cw, work, out3)
    else:
        call("u2pl_ce_fwd_f32", xc, td, IGN, N, C, Hh, W, int(unsup), work, out3)
    return dict(loss=float(loss.detach()), out3=out3.cpu().numpy(), grad=x.grad)


def check_ce(zd, td, sm, C, zmax, unsup, cw, gmul, gout, tag):
    ref = LB.ce_ref(zd, td, unsup_weight=unsup, class_weight=cw, gout=gout, gmul=gmul, sm=sm)
    got = device_ce(zd, td, unsup, cw, gmul, gout)
    ex = LB.ce_excess(got, ref, C, zmax, gmul)
    assert max(ex.values()) <= 1.0, (tag, ex, got["out3"], ref["out3"])
    return ex


def weights(C):
    return D(LB.seeded_weights(C))


# ------------------------------------------------------------------ cross entropy
@pytest.mark.parametrize("C,shape", CS, ids=CS_IDS)
def test_ce_forward_backward_every_family_and_ignore_pattern(C, shape):
    """loss and the WHOLE gradient inside the bound, out3[2] exactly n_valid / the fp32 weight sum, ignored pixels' gradient
    exactly 0; everything ignored: NaN loss and a gradient of zeros only; weights summing to zero on valid pixels: NaN there"""
    worst = {}
    for fam in LB.FAMILIES:
        c = case(fam, C, shape)
        for pat in LB.IGNORES:
            t, td = target(fam, C, shape, pat)
            for name, unsup, weighted, gmul, gout in CE_FORMS:
                ex = check_ce(c["zd"], td, c["sm"], C, c["zmax"], unsup, weights(C) if weighted else None, gmul, gout, (fam, pat, name))
                for k, v in ex.items():
                    worst[k] = max(worst.get(k, 0.0), v)
            if pat == "all":
                g = device_ce(c["zd"], td, False, None, 1.0, 1.0)
                assert math.isnan(g["loss"]) and math.isnan(g["out3"][0]) and g["out3"][2] == 0 and not bool(g["grad"].any())
    print(f"\nC={C} {shape}: worst excess " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()), end="")


@pytest.mark.parametrize("gmul", [1.0, 0.4])
@pytest.mark.parametrize("gout", [1.0, 1.7, -0.6])
def test_ce_scaling(gmul, gout):
    for name, unsup, weighted, _, _ in CE_FORMS:
        for fam in ("trained", "wrong"):
            c = case(fam, 21, (3, 23, 31))
            _, td = target(fam, 21, (3, 23, 31), "some")
            check_ce(c["zd"], td, c["sm"], 21, c["zmax"], unsup, weights(21) if weighted else None, gmul, gout, (fam, name, gmul, gout))


def test_ce_class_weights_of_the_reference_and_a_zero_weight():
    """the reference's CE_CLASS_WEIGHT (nine exact zeros) and OHEM_CLASS_WEIGHT at C = 19, a seeded vector with an exact 0 at 150"""
    from u2pl_amd.utils import loss_helper as LH
    for C, ws in ((19, (LH.CE_CLASS_WEIGHT, LH.OHEM_CLASS_WEIGHT)), (150, (LB.seeded_weights(150),))):
        for w in ws:
            w = np.asarray(w, dtype=np.float32)
            assert (w == 0).any() or C == 19
            for fam in LB.FAMILIES:
                for shape in ((3, 23, 31), (2, 65, 65)):
                    c = case(fam, C, shape)
                    for pat in ("none", "some", "image"):
                        _, td = target(fam, C, shape, pat)
                        for gmul, gout in ((1.0, 1.0), (0.4, 1.7)):
                            check_ce(c["zd"], td, c["sm"], C, c["zmax"], False, D(w), gmul, gout, (C, fam, shape, pat))


@pytest.mark.parametrize("layout", ["channels_last", "sliced_channels", "sliced_width"])
def test_ce_layouts_give_the_bits_of_a_contiguous_input(layout):
    """the wrapper's .contiguous(): a channels-last or sliced logits tensor gives the same loss and gradient bits"""
    H = hip()
    C, shape = 19, (3, 23, 31)
    c = case("trained", C, shape)
    _, td = target("trained", C, shape, "some")
    zc = c["zd"]
    if layout == "channels_last":
        zl = zc.contiguous(memory_format=torch.channels_last)
    elif layout == "sliced_channels":
        zl = torch.randn(3, C + 5, 23, 31, device=DEV)[:, 2:2 + C]
        zl.copy_(zc)
    else:
        zl = torch.randn(3, C, 23, 40, device=DEV)[..., 4:35]
        zl.copy_(zc)
    assert not zl.is_contiguous() and torch.equal(zl, zc)
    outs = []
    for z in (zc, zl):
        for kw in (dict(), dict(unsup_weight=True, scale=0.4), dict(class_weight=weights(C))):
            x = z.detach().requires_grad_(True)
            loss = H.cross_entropy(x, td, IGN, **kw)
            loss.backward(torch.tensor(1.7, device=DEV))
            outs.append((loss.detach().clone(), x.grad.contiguous()))
    for (l0, g0), (l1, g1) in zip(outs[:3], outs[3:]):
        assert torch.equal(l0.view(torch.int32), l1.view(torch.int32)) and torch.equal(g0.view(torch.int32), g1.view(torch.int32))


# ------------------------------------------------------------------ OHEM
def device_ohem_prob(zd, td):
    H = hip()
    N, C, Hh, W = zd.shape
    ws = H.new_select_ws(DEV, N * Hh * W)
    mp = torch.full((N, Hh, W), -7.0, dtype=torch.float32, device=DEV)
    call("u2pl_ohem_prob_f32", zd.contiguous(), td, IGN, N, C, Hh, W, mp, ws)
    return mp, ws


def check_ohem(fam, C, shape, pats=LB.IGNORES):
    H = hip()
    c = case(fam, C, shape)
    nrule = 0
    for pat in pats:
        t, td = target(fam, C, shape, pat)
        valid = td != IGN
        mp64, nv, _, _ = LB.ohem_ref(c["zd"], td, 0.7, 1, sm=c["sm"])
        mp, ws = device_ohem_prob(c["zd"], td)
        assert LB._nan_aware_excess(mp, mp64, LB.E_prob(C)) <= 1.0, (fam, pat)
        assert bool((mp[~valid] == 1.0).all())
        wsn = ws.cpu().numpy()
        assert int(wsn[0]) == nv == int((t != IGN).sum())
        assert np.array_equal(wsn[128:128 + 2048], LB.hist0_of(mp.cpu().numpy()))
        srt, srt64 = torch.sort(mp.reshape(-1)).values, torch.sort(mp64.reshape(-1)).values
        for thresh in (0.0, 0.7, 1.0):
            for mk in sorted({0, 1, nv // 3, nv, nv + 1}):      # (0: the reference drops nothing)
                kept = H.ohem_kept_target(c["zd"], td, thresh, mk, IGN)
                # exactly the rule on the device's own mask_prob and the threshold that the reference's rule takes from it
                thr = LB.ohem_threshold(mp, nv, thresh, mk, srt)
                assert torch.equal(kept, LB.ohem_rule(mp, thr, td)), (fam, pat, thresh, mk, thr)
                # the float64 rule: a kept target may differ only where |p64 - thr64| is inside the bound
                thr64 = LB.ohem_threshold(mp64, nv, thresh, mk, srt64)
                if LB.ohem_rule_checked(fam, nv, thr64, thresh):
                    band = LB.ohem_band(mp64, thr64, valid, C, thresh)
                    assert int(band.sum()) <= LB.OHEM_RULE_CAP * nv, (fam, pat, thresh, mk, int(band.sum()), nv)
                    assert not bool(((kept != LB.ohem_rule(mp64, thr64, td)) & ~band).any()), (fam, pat, thresh, mk)
                    nrule += 1
    return nrule


@pytest.mark.parametrize("C,shape", CS, ids=CS_IDS)
def test_ohem_probability_and_kept_target(C, shape):
    """mask_prob inside the bound (1.0 on ignored pixels), ws[0] and the pass-0 histogram exact, the kept target exactly the
    rule for min_kept in {0, 1, n_valid // 3, n_valid, n_valid + 1} x thresh in {0, 0.7, 1}, and the float64 rule outside its band"""
    nrule = sum(check_ohem(fam, C, shape) for fam in LB.FAMILIES)
    assert nrule >= (15 if shape == (2, 65, 65) else 1)


# ------------------------------------------------------------------ pseudo label
@pytest.mark.parametrize("C,shape", CS, ids=CS_IDS)
def test_pseudo_label(C, shape):
    """labels exactly np.argmax on every pixel (no gap mask: arg-max over fp32 inputs is exact, ties go to the lowest index),
    conf inside the bound"""
    H = hip()
    for fam in LB.FAMILIES:
        c = case(fam, C, shape)
        conf, label = H.pseudo_label(c["zd"])
        assert np.array_equal(label.cpu().numpy(), c["argmax"]), fam
        assert LB._nan_aware_excess(conf, c["sm"][0].amax(1), LB.E_prob(C)) <= 1.0, fam


# ------------------------------------------------------------------ entropy
def check_entropy_outputs(ent, ws, ref64, label, C, tag):
    """values inside the bound, NaN exactly on ignored pixels, ws[0] and the 2048-bin histogram exact (from the output's own bits)"""
    valid = torch.ones_like(ent, dtype=torch.bool) if label is None else label != IGN
    assert torch.equal(torch.isnan(ent), ~valid), tag
    e = LB._nan_aware_excess(ent[valid], ref64[valid], LB.E_ent(C)) if bool(valid.any()) else 0.0
    assert e <= 1.0, (tag, e)
    if C <= 33 and bool(valid.any()):      # the stated 2e-6 tolerance, where fp32 arithmetic can keep it (FINDING 3)
        assert float((ent[valid].double() - ref64[valid]).abs().max()) <= LB.CONTRACT_ENTROPY, tag
    wsn = ws.cpu().numpy()
    assert int(wsn[0]) == int(valid.sum()), tag
    assert np.array_equal(wsn[128:128 + 2048], LB.hist0_of(ent.cpu().numpy())), tag
    return e


@pytest.mark.parametrize("C,shape", CS, ids=CS_IDS)
def test_entropy_map(C, shape):
    H = hip()
    for fam in LB.FAMILIES:
        c = case(fam, C, shape)
        ref = LB.entropy_ref(c["zd"], c["sm"])
        for pat in (None, "some", "image", "one", "all"):
            td = None if pat is None else target(fam, C, shape, pat)[1]
            ws = H.new_select_ws(DEV, int(np.prod(shape)))
            ent = H.entropy_map(c["zd"], td, ws)
            check_entropy_outputs(ent, ws, ref, td, C, (fam, pat))


# route -> (C, low size, size): the generic kernels at a size that is not 4x, the 4x size with class counts that must fall to
# <0>, the LDS cell kernels square and not, a 1 x 1 input
UP_ROUTES = [("up19", 19, (5, 7), (17, 23)), ("up21", 21, (5, 7), (17, 23)), ("up0", 33, (5, 7), (17, 23)),
             ("up0_at_4x", 20, (17, 17), (65, 65)), ("up0_at_4x", 33, (9, 13), (33, 49)), ("up0_at_4x", 150, (9, 13), (33, 49)),
             ("cell_lds19", 19, (17, 17), (65, 65)), ("cell_lds21", 21, (17, 17), (65, 65)),
             ("cell_lds19", 19, (9, 13), (33, 49)), ("cell_lds21", 21, (9, 13), (33, 49)),
             ("one_pixel", 19, (1, 1), (4, 5)), ("one_pixel", 21, (1, 1), (1, 1)), ("one_pixel", 7, (1, 1), (3, 2))]


@pytest.mark.parametrize("route,C,lo,hi", UP_ROUTES, ids=[f"{r}-C{C}-{lo[0]}x{lo[1]}" for r, C, lo, hi in UP_ROUTES])
@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
def test_entropy_map_up_routes(route, C, lo, hi, layout):
    """entropy_map_up is entropy_map(bilinear_up(...)) bit for bit (values, ws[0], histogram) on every route and layout, and
    inside the float64 bound of the up-sampled logits"""
    H = hip()
    N = 3
    for fam in ("trained", "ties", "saturated"):
        low = D(LB.make_case(fam, C, (N,) + lo)[0])
        if layout == "nhwc":
            low = low.contiguous(memory_format=torch.channels_last)
        large = H.bilinear_up(low, hi)
        assert np.array_equal(large.cpu().numpy(), R.bilinear_ac(low.cpu().numpy(), *hi))
        ref = LB.entropy_ref(large)
        lab = LB.apply_ignore(np.zeros((N,) + hi, dtype=np.int64), "some")
        for td in (None, D(lab)):
            ws1, ws2 = H.new_select_ws(DEV, N * hi[0] * hi[1]), H.new_select_ws(DEV, N * hi[0] * hi[1])
            e1 = H.entropy_map(large, td, ws1)
            e2 = H.entropy_map_up(low, hi, td, ws2)
            assert torch.equal(e1.view(torch.int32), e2.view(torch.int32)), (route, fam)
            assert torch.equal(ws1[:128 + 2048], ws2[:128 + 2048])
            check_entropy_outputs(e2, ws2, ref, td, C, (route, fam))


# ------------------------------------------------------------------ confusion histogram
def device_confusion(zd, td, C):
    N, _, Hh, W = zd.shape
    hist = torch.zeros(3 * C, dtype=torch.int64, device=DEV)
    call("u2pl_confusion_hist_f32", zd.contiguous(), td, IGN, N, C, Hh, W, hist)
    return hist.cpu().reshape(3, C)


@pytest.mark.parametrize("C", [2, 19, 150, 255])
def test_confusion_histogram(C):
    """exact integers, lowest-index arg-max on ties; labels in [C, 255) that are not the ignore value count in area_output only"""
    for shape in LB.SHAPES:
        for fam in ("trained", "ties", "uniform"):
            c = case(fam, C, shape)
            for pat in LB.IGNORES:
                t = target(fam, C, shape, pat)[0].copy()
                if C < 254:
                    rng = np.random.default_rng(C)
                    out = rng.random(t.shape) < 0.1
                    t[out & (t != IGN)] = rng.integers(C, 255, t.shape)[out & (t != IGN)]
                ref = LB.confusion_ref(c["z"], t, C)
                assert torch.equal(device_confusion(c["zd"], D(t), C), ref), (shape, fam, pat)
                if C < 254 and pat == "none" and t.size > 50:
                    assert int(ref[1].sum()) > int(ref[2].sum())


# ------------------------------------------------------------------ bilinear backward
@pytest.mark.parametrize("lo,hi", LB.BIL_SHAPES, ids=[f"{lo[0]}x{lo[1]}-{hi[0]}x{hi[1]}" for lo, hi in LB.BIL_SHAPES])
@pytest.mark.parametrize("C", [1, 5, 19])
@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
def test_bilinear_up_backward(lo, hi, C, layout):
    """inside the bound of the float64 transpose of the forward's own coordinates, and the adjoint identity <g, up(x)> =
    <bwd(g), x> in float64"""
    H = hip()
    rng = np.random.default_rng([C, lo[0], hi[1]])
    x = rng.standard_normal((2, C) + lo).astype(np.float32)
    g = rng.standard_normal((2, C) + hi).astype(np.float32)
    xd = D(x)
    if layout == "nhwc":
        xd = xd.contiguous(memory_format=torch.channels_last)
    xd.requires_grad_(True)
    up = H.bilinear_up(xd, hi)
    up.backward(D(g))
    gin = xd.grad.cpu().numpy()
    assert LB.bil_excess(gin, g, *lo) <= 1.0
    Ay, Ax = LB.ac_matrix(hi[0], lo[0]), LB.ac_matrix(hi[1], lo[1])
    lhs = float((g.astype(np.float64) * up.detach().cpu().numpy().astype(np.float64)).sum())
    rhs = float((gin.astype(np.float64) * x.astype(np.float64)).sum())
    size = float((np.abs(g) * LB.bilinear_fwd64(np.abs(x), *hi)).sum())
    assert abs(lhs - rhs) <= (LB.E_bil(Ay, Ax) + 3 * LB.EPS) * size


# ------------------------------------------------------------------ the second grid-stride trip
def test_grid_stride_shapes_pass_each_cap():
    for cap, (N, Hh, W) in LB.STRIDE_SHAPES.items():
        assert cap * 256 < N * Hh * W < cap * 256 * 1.01
    assert set(LB.GRID_CAPS.values()) == set(LB.STRIDE_SHAPES)


@pytest.mark.parametrize("cap", sorted(LB.STRIDE_SHAPES))
def test_grid_stride(cap):
    """C = 3, N = 2 just over each launch cap: the same assertions as above, for the kernels that the cap belongs to"""
    H = hip()
    C, shape = 3, LB.STRIDE_SHAPES[cap]
    fam = "trained"
    c = case(fam, C, shape)
    t, td = target(fam, C, shape, "some")
    if cap == 512:
        assert check_ohem(fam, C, shape, pats=("some",)) == 15
        ref = LB.entropy_ref(c["zd"], c["sm"])
        ws = H.new_select_ws(DEV, t.size)
        check_entropy_outputs(H.entropy_map(c["zd"], td, ws), ws, ref, td, C, "k_entropy")
        lo = ((shape[1] + 3) // 4, shape[2] // 4)
        low = D(LB.make_case(fam, C, (2,) + lo)[0])
        large = H.bilinear_up(low, shape[1:])
        ws1, ws2 = H.new_select_ws(DEV, t.size), H.new_select_ws(DEV, t.size)
        e1, e2 = H.entropy_map(large, td, ws1), H.entropy_map_up(low, shape[1:], td, ws2)
        assert torch.equal(e1.view(torch.int32), e2.view(torch.int32)) and torch.equal(ws1[:128 + 2048], ws2[:128 + 2048])
        check_entropy_outputs(e2, ws2, LB.entropy_ref(large), td, C, "k_entropy_up")
        tc = t.copy()
        tc[0, :5] = 77
        assert torch.equal(device_confusion(c["zd"], D(tc), C), LB.confusion_ref(c["z"], tc, C))
    else:      # 2048: k_ce_fwd; 4096: k_ce_bwd as well, k_pseudo_label, k_bilinear_up
        for name, unsup, weighted, gmul, gout in CE_FORMS:
            check_ce(c["zd"], td, c["sm"], C, c["zmax"], unsup, weights(C) if weighted else None, gmul, gout, name)
    if cap == 4096:
        conf, label = H.pseudo_label(c["zd"])
        assert np.array_equal(label.cpu().numpy(), c["argmax"])
        assert LB._nan_aware_excess(conf, c["sm"][0].amax(1), LB.E_prob(C)) <= 1.0
        low = LB.make_case(fam, C, (2, 182, 181))[0]
        assert np.array_equal(H.bilinear_up(D(low), shape[1:]).cpu().numpy(), R.bilinear_ac(low, *shape[1:]))
