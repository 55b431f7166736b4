"""The loss-head bounds of tests/loss_bounds.py on the CPU: the float64 references are pinned to oracle/restate.py, to
tests/reliability_ref.py and to torch's float64 autograd; the calibrated ceilings are re-measured from the reference's own fp32
arithmetic (-s prints them); the numpy fp32 emulation of every kernel in its own order and torch fp32 meet the bounds on every
logit family; each faulty emulation is rejected on a named family and shape; the float64 OHEM rule with the bound applied to itself
leaves out at most 0.1 % of the valid pixels of a checked case.  (The GPU kernels are held to the same bounds in
tests/test_gpu_loss_bounds.py.)"""
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_bounds as LB  # noqa: E402
import reliability_ref as RR  # noqa: E402
from oracle import restate as R  # noqa: E402

f32 = np.float32
T = torch.from_numpy


# ------------------------------------------------------------------ one truth: the references against the existing ones
@pytest.mark.parametrize("family", ["trained", "ties", "offset"])
def test_ce_reference_is_the_oracles_and_torch_float64(family):
    C, shape = 19, (2, 9, 11)
    z, tgt = LB.make_case(family, C, shape)
    cw = LB.seeded_weights(C)
    for pat in LB.IGNORES[:4]:
        t = LB.apply_ignore(tgt, pat)
        ref = LB.ce_ref(z, t)
        lo = R.cross_entropy_mean(z, t)
        assert abs(ref["loss"] - lo) <= 1e-12 * max(1.0, abs(lo))
        assert ref["out3"][2] == (t != 255).sum()
        for kw in (dict(), dict(unsup_weight=True, gout=1.7, gmul=0.4), dict(class_weight=cw, gout=-0.6, gmul=0.4)):
            ref = LB.ce_ref(z, t, **kw)
            if not ref["out3"][2] > 0:
                continue
            zt = T(z).double().requires_grad_(True)
            w = None if "class_weight" not in kw else T(cw).double()
            loss = F.cross_entropy(zt, T(t), weight=w, ignore_index=255)
            if kw.get("unsup_weight"):
                loss = loss * (t.size / (t != 255).sum())       # loss_helper.py:44
            loss = loss * kw.get("gmul", 1.0)
            loss.backward(torch.tensor(kw.get("gout", 1.0), dtype=torch.float64))
            assert abs(float(loss.detach()) - ref["loss"]) <= 1e-12 * max(1.0, abs(ref["loss"]))
            assert float((zt.grad - ref["grad"]).abs().max()) <= 1e-13 * float(ref["scale"].abs().max())
            if w is not None:
                assert abs(ref["out3"][2] - float((w[T(np.where(t != 255, t, 0))] * T(t != 255)).sum())) < 1e-9


def test_everything_ignored_is_nan_loss_and_zero_gradient():
    """what k_ce_finish documents and torch CPU does"""
    z, tgt = LB.make_case("trained", 19, (2, 5, 7))
    t = LB.apply_ignore(tgt, "all")
    for kw in (dict(), dict(unsup_weight=True), dict(class_weight=LB.seeded_weights(19))):
        for impl in (LB.ce_ref, LB.torch_ce_fp32, LB.emu_ce):
            out = impl(z, t, **kw)
            assert math.isnan(float(out["loss"])) and not LB._T(out["grad"]).any(), (impl.__name__, kw)
        assert max(LB.ce_excess(LB.emu_ce(z, t, **kw), LB.ce_ref(z, t, **kw), 19, 10.0).values()) == 0.0


def test_ohem_entropy_pseudo_references_are_the_oracles():
    C, shape = 19, (2, 23, 31)
    z, tgt = LB.make_case("trained", C, shape)
    t = LB.apply_ignore(tgt, "some")
    nv = int((t != 255).sum())
    for thresh, mk in ((0.7, nv // 3), (0.7, 1), (0.0, nv // 3), (1.0, nv), (0.7, nv + 1), (0.7, 0)):
        mp, n, thr, kept = LB.ohem_ref(z, t, thresh, mk)
        _, kept_o, used = R.ohem_ce(z, t, thresh, mk)
        assert n == nv
        if used is None or mk == 0:          # nothing dropped (the oracle reports the fixed threshold at min_kept = 0 and keeps all)
            assert math.isinf(thr) and np.array_equal(kept.numpy(), t) and np.array_equal(kept_o, t)
            continue
        assert abs(thr - float(used)) <= 2 * LB.E_prob(C)
        diff = T(kept_o) != kept             # the oracle's softmax is fp32: a pixel may flip only inside the band
        assert not bool((diff & ~LB.ohem_band(mp, thr, T(t != 255), C, thresh)).any())
    # entropy: the reference expression of reliability_ref in float64, the oracle's in fp32
    e = LB.entropy_ref(z).numpy()
    assert np.abs(e - RR.entropy_ref64(z)).max() <= 1e-13
    assert np.abs(e - R.entropy_from_logits(z)).max() <= LB.E_ent(C)
    # the two emulations of k_entropy (numpy's fp32 exp / log there, correctly rounded ones here) agree to a few roundings
    assert np.abs(RR.entropy_logits_f32(z) - LB.emu_entropy(z)).max() <= 8 * LB.EPS * math.log(C)
    # pseudo label: first maximum
    conf, lab = LB.pseudo_ref(z)
    co, lo = R.pseudo_label(z)
    assert np.array_equal(lab.numpy(), lo) and np.abs(conf.numpy() - co).max() <= LB.E_prob(C)
    zt, _ = LB.make_case("ties", C, shape)
    assert np.array_equal(LB.pseudo_ref(zt)[1].numpy(), R.pseudo_label(zt)[1])
    dup = (zt == zt.max(1, keepdims=True)).sum(1)
    assert (dup >= 2).all() and (dup == C).any() and (dup >= 3).any()      # the family holds what it promises


def test_confusion_reference_and_histogram_key():
    z, tgt = LB.make_case("ties", 5, (3, 7, 9))
    t = LB.apply_ignore(tgt, "some")
    t[0, 0, :4] = (5, 77, 254, 6)            # labels outside [0, C) that are not the ignore value
    h = LB.confusion_ref(z, t, 5).numpy()
    am = z.argmax(1)
    live = t != 255
    inside = live & (t < 5)
    assert np.array_equal(h[1], np.bincount(am[live], minlength=5)) and np.array_equal(h[2], np.bincount(t[inside], minlength=5))
    assert np.array_equal(h[0], np.bincount(t[inside & (am == t)], minlength=5)) and h[1].sum() == h[2].sum() + 4
    ai, au, at = R.intersection_and_union(np.where(live, am, 255), t, 5)
    assert np.array_equal(h[0], ai) and np.array_equal(h[2], at) and np.array_equal(h[1] + h[2] - h[0], au)
    v = np.array([0.0, 1.0, -1.0, 3.5e-5, np.nan, np.inf], dtype=f32)
    v[4] = np.frombuffer(np.uint32(0x7fc00000).tobytes(), dtype=f32)[0]
    hist = LB.hist0_of(v)
    assert hist.sum() == 6 and hist[0x7fc00000 >> 21 | 1024] == 1 and hist[1024] == 1 and hist[(0x3f800000 >> 21) | 1024] == 1
    assert hist[((~np.uint32(0xbf800000)) >> np.uint32(21))] == 1


@pytest.mark.parametrize("lo,hi", LB.BIL_SHAPES)
def test_bilinear_coordinates_are_the_forwards_bit_for_bit(lo, hi):
    """ac_matrix holds the forward's own (i0, i1, l0, l1): rounded to fp32 it IS oracle.restate.bilinear_ac of the unit rows (a
    1-wide image: the x taps are (1, 0) exactly); the float64 forward is the oracle's within three roundings, the float64 backward
    is torch's float64 one up to the float64 rounding of the fp32 coordinates, and the adjoint identity holds"""
    for n_in, n_out in ((lo[0], hi[0]), (lo[1], hi[1])):
        A = LB.ac_matrix(n_out, n_in)
        unit = np.eye(n_in, dtype=f32).reshape(n_in, 1, n_in, 1)
        assert np.array_equal(A.astype(f32), R.bilinear_ac(unit, n_out, 1)[:, 0, :, 0].T)
        assert np.abs(A.sum(1) - 1).max() <= LB.EPS
    rng = np.random.default_rng(7)
    x = rng.standard_normal((2, 3) + lo).astype(f32)
    g = rng.standard_normal((2, 3) + hi).astype(f32)
    up64 = LB.bilinear_fwd64(x, *hi)
    assert np.abs(up64 - R.bilinear_ac(x, *hi)).max() <= 3 * LB.EPS * np.abs(x).max()
    b64, unit = LB.bilinear_bwd64(g, *lo)
    assert abs((g * up64).sum() - (b64 * x).sum()) <= 1e-12 * (np.abs(g) * LB.bilinear_fwd64(np.abs(x), *hi)).sum()
    xt = T(x).double().requires_grad_(True)
    F.interpolate(xt, hi, mode="bilinear", align_corners=True).backward(T(g).double())
    assert np.abs(xt.grad.numpy() - b64).max() <= 4 * LB.EPS * unit.max()       # torch's float64 lambdas differ from the fp32 ones
    for form in ("torch", "emu"):
        got = LB.torch_bilinear_bwd_fp32(g, *lo) if form == "torch" else LB.emu_bilinear_bwd(g, *lo)
        assert LB.bil_excess(got, g, *lo) <= 1.0, form


# ------------------------------------------------------------------ the calibration, re-measured
CEIL = {}


@pytest.mark.parametrize("C", LB.CLASSES)
def test_ceilings_and_both_fp32_forms_meet_the_bounds(C):
    """re-measures the ceilings beside the CAL_* constants (torch fp32 = the reference's formulas, never a HIP kernel) and holds
    torch fp32 and the faithful emulation to the asserted bounds on every family"""
    cals = dict(grad=LB.cal_grad(C), loss=LB.cal_loss(C), prob=LB.cal_prob(C), ent=LB.cal_ent(C))
    bounds = dict(grad=LB.E_grad(C) / LB.EPS, prob=LB.E_prob(C) / LB.EPS,
                  ent=(LB.E_ent(C) - C * LB.LOG_DELTA) / (LB.EPS * max(1.0, math.log(C))),
                  loss=min(LB.loss_count(C), LB.CAL_MARGIN * LB.cal_loss(C)))
    for form in ("torch", "emu"):
        worst = dict(grad=0.0, loss=0.0, prob=0.0, ent=0.0)
        for fam in LB.FAMILIES:
            m = LB.measure_case(fam, C, form=form)
            print(f"\n{form:5s} C={C:3d} {fam:9s} " + " ".join(f"{k} {v:6.2f}" for k, v in m.items()), end="")
            for k, v in m.items():
                worst[k] = max(worst[k], v)
                slack = C * LB.LOG_DELTA / (LB.EPS * max(1.0, math.log(C))) if k == "ent" else 0.0
                assert v <= bounds[k] + slack, (form, fam, C, k, v, bounds[k])
        print(f"\n{form:5s} C={C:3d} ceiling   " + " ".join(f"{k} {v:6.2f}" for k, v in worst.items())
              + "   calibrated " + " ".join(f"{k} {v:6.2f}" for k, v in cals.items()))
        if form == "torch":
            for k, v in worst.items():          # the constants are ceilings of the measurement, and not padded ones
                assert v <= cals[k] and (C not in (2, 255) or k == "loss" or v >= 0.45 * cals[k]), (k, v, cals[k])


def test_bilinear_ceiling():
    worst = {}
    for form in ("torch", "emu"):
        worst[form] = [LB.measure_bilinear(lo, hi, form) for lo, hi in LB.BIL_SHAPES]
        print(f"\n{form:5s} bilinear backward " + " ".join(f"{v:5.2f}" for v in worst[form]), end="")
    assert max(worst["torch"]) <= LB.CAL_BIL and max(worst["emu"]) <= LB.CAL_MARGIN * LB.CAL_BIL
    assert max(worst["torch"]) >= 0.5 * LB.CAL_BIL


def test_findings_derived_count_against_calibration_and_contracts():
    """the FINDINGS of the module docstring, as assertions"""
    # 1: the first-order count is the smaller bound at the small class counts, the calibrated one at the large
    assert [LB.grad_count(C) < LB.CAL_MARGIN * LB.cal_grad(C) for C in LB.CLASSES] == [True, True, True, True, True, False]
    assert [LB.prob_count(C) < LB.CAL_MARGIN * LB.cal_prob(C) for C in LB.CLASSES] == [True, True, True, True, True, False]
    assert [LB.loss_count(C) < LB.CAL_MARGIN * LB.cal_loss(C) for C in LB.CLASSES] == [True, True, True, True, False, False]
    assert [LB.ent_count(C) < LB.CAL_MARGIN * LB.cal_ent(C) for C in LB.CLASSES] == [True, False, False, False, False, False]
    # 2: "fp32 losses within 1e-4" is the smaller bound once max|z| reaches a few tens (saturated, offset): E_loss takes it
    assert LB.E_loss(19, 1.0) < LB.CONTRACT_LOSS < LB.E_loss(19, 100.0) and LB.E_loss(19, 1000.0, 1.0, 3.0) == LB.CONTRACT_LOSS * 3.0
    # 3: the 2e-6 entropy tolerance is above the bound up to 33 classes and BELOW what fp32 arithmetic reaches at 150 and 255:
    # the reference's own fp32 expression misses it there (9.81 and 13.95 units of EPS ln C = 2.9e-6 and 4.6e-6)
    assert all(LB.CAL_MARGIN ** -1 * LB.E_ent(C) < LB.CONTRACT_ENTROPY for C in (2, 19, 21, 33))
    for C, fam in ((150, "uniform"), (255, "ties")):
        z, _ = LB.make_case(fam, C, LB.CAL_SHAPE)
        err = float((LB.torch_entropy_fp32(z).double() - LB.entropy_ref(z)).abs().max())
        assert LB.CONTRACT_ENTROPY < err <= LB.E_ent(C), (C, err)


# ------------------------------------------------------------------ the bounds must be able to fail
S1 = (2, 23, 31)
FAULT_CASES = {      # fault -> (head, family, C, shape, ignore pattern)
    "drop_last_class": [("ce", "uniform", 19, S1, "some"), ("ohem", "uniform", 19, S1, "some"), ("pseudo", "uniform", 19, S1, None),
                        ("entropy", "uniform", 19, S1, None), ("ce", "trained", 255, S1, "none")],
    # (softmax does not depend on the shift: a maximum that misses the last class shows where expf overflows, and in the arg-max)
    "max_over_C-1": [("ce", "saturated", 2, S1, "none"), ("ohem", "saturated", 2, S1, "none"), ("pseudo", "trained", 19, S1, None),
                     ("entropy", "saturated", 2, S1, None)],
    "batch_offset_n_HW": [("ce", "trained", 19, S1, "some"), ("ohem", "trained", 2, S1, "none"), ("pseudo", "trained", 19, S1, None),
                          ("entropy", "trained", 19, S1, None)],
    "skip_pixel_65536": [("ce", "trained", 3, (2, 257, 256), "some"), ("ohem", "trained", 3, (2, 257, 256), "some"),
                         ("pseudo", "trained", 3, (2, 257, 256), None), ("entropy", "trained", 3, (2, 257, 256), None)],
    "count_ignored": [("ce", "trained", 19, S1, "some"), ("ce", "trained", 19, S1, "one")],
    "weight_at_argmax": [("ce_w", "wrong", 19, S1, "some"), ("ce_w", "trained", 150, S1, "none")],
    "gmul_twice": [("ce", "trained", 19, S1, "some")],
    "entropy_no_t_over_s": [("entropy", "uniform", 19, S1, None), ("entropy", "trained", 255, S1, None)],
    "argmax_highest_tie": [("pseudo", "ties", 19, S1, None), ("pseudo", "ties", 2, (1, 7, 9), None)],
    "bilinear_skip_i1_eq_i0": [("bilinear", None, 5, ((5, 7), (17, 23)), None), ("bilinear", None, 5, ((1, 1), (4, 5)), None)],
}


def _head_excess(head, family, C, shape, pat, fault):
    """the largest excess of the emulation (faithful or faulty) of one head on one case"""
    if head == "bilinear":
        lo, hi = shape
        g = np.random.default_rng(5).standard_normal((2, C) + hi).astype(f32)
        return LB.bil_excess(LB.emu_bilinear_bwd(g, *lo, fault=fault), g, *lo)
    z, tgt = LB.make_case(family, C, shape)
    zmax = float(np.abs(z).max())
    sm = LB.softmax64(z)
    if head in ("ce", "ce_w"):
        t = LB.apply_ignore(tgt, pat)
        worst = 0.0
        kws = [dict(class_weight=LB.seeded_weights(C), gout=1.7, gmul=0.4)] if head == "ce_w" else \
            [dict(), dict(unsup_weight=True, gout=1.7, gmul=0.4)]
        for kw in kws:
            ex = LB.ce_excess(LB.emu_ce(z, t, fault=fault, **kw), LB.ce_ref(z, t, sm=sm, **kw), C, zmax, kw.get("gmul", 1.0))
            worst = max(worst, max(ex.values()))
        return worst
    if head == "ohem":
        t = LB.apply_ignore(tgt, pat)
        mp64, nv, _, _ = LB.ohem_ref(z, t, 0.7, 1, sm=sm)
        mp, n = LB.emu_ohem_prob(z, t, fault=fault)
        return math.inf if n != nv else LB._nan_aware_excess(mp, mp64, LB.E_prob(C))
    if head == "pseudo":
        conf64, lab = LB.pseudo_ref(z, sm)
        conf, l = LB.emu_pseudo(z, fault=fault)
        return math.inf if not np.array_equal(l, lab.numpy()) else LB._nan_aware_excess(conf, conf64, LB.E_prob(C))
    assert head == "entropy"
    return LB._nan_aware_excess(LB.emu_entropy(z, fault=fault), LB.entropy_ref(z, sm), LB.E_ent(C))


@pytest.mark.parametrize("fault", LB.FAULTS)
def test_bound_rejects_fault(fault):
    """every named case passes with the faithful emulation and fails with the faulty one"""
    for head, family, C, shape, pat in FAULT_CASES[fault]:
        good, bad = _head_excess(head, family, C, shape, pat, None), _head_excess(head, family, C, shape, pat, fault)
        print(f"\n{fault:24s} {head:8s} {str(family):9s} C={C:3d} {shape} {pat}: faithful {good:.3f} faulty {bad:.3g}", end="")
        assert good <= 1.0 < bad, (fault, head, family, C, shape, pat, good, bad)


def test_every_fault_is_covered():
    assert set(FAULT_CASES) == set(LB.FAULTS)


# ------------------------------------------------------------------ the one comparison that may leave pixels out
def test_ohem_float64_rule_band_stays_under_the_cap():
    """the float64 reference with the bound applied to itself: on every case that the GPU test checks against the float64 rule
    (loss_bounds.ohem_rule_checked) the band holds at most 0.1 % of the valid pixels; the other families show why they are left to
    the exact device-rule check"""
    checked = 0
    for C, shape in [(C, shape) for C in LB.CLASSES for shape in LB.SHAPES] + [(3, LB.STRIDE_SHAPES[512])]:
        for fam in LB.RULE_FAMILIES:
            z, tgt = LB.make_case(fam, C, shape)
            sm = LB.softmax64(z)
            for pat in LB.IGNORES:
                t = LB.apply_ignore(tgt, pat)
                nv = int((t != 255).sum())
                mp = LB.ohem_ref(z, t, 0.7, 1, sm=sm)[0]
                srt = torch.sort(mp.reshape(-1)).values
                for thresh in (0.0, 0.7, 1.0):
                    for mk in sorted({0, 1, nv // 3, nv, nv + 1}):
                        thr = LB.ohem_threshold(mp, nv, thresh, mk, srt)
                        if not LB.ohem_rule_checked(fam, nv, thr, thresh):
                            continue
                        band = int(LB.ohem_band(mp, thr, T(t != 255), C, thresh).sum())
                        assert band <= LB.OHEM_RULE_CAP * nv, (fam, C, shape, pat, thresh, mk, band, nv)
                        checked += 1
    assert checked > 900
    z, tgt = LB.make_case("uniform", 19, (2, 65, 65))
    mp, nv, thr, _ = LB.ohem_ref(z, tgt, 0.0, tgt.size // 3)
    assert int(LB.ohem_band(mp, thr, T(tgt != 255), 19, 0.0).sum()) > 0.01 * nv
