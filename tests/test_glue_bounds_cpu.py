"""The glue-kernel bounds of tests/glue_bounds.py on the CPU: the float64 references are pinned to torch float64 and, where one
exists, to oracle/restate.py; the calibrated ceilings are re-measured from torch's own fp32 arithmetic (-s -k ceilings prints
them); the numpy fp32 emulation of every kernel in its own order and torch fp32 meet every bound; each named faulty emulation is
rejected on a named family and shape.  (The GPU kernels are held to the same bounds in tests/test_gpu_glue_bounds.py.)"""
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import glue_bounds as GB  # noqa: E402
from oracle import restate as R  # noqa: E402

f32, f64 = np.float32, np.float64
T = torch.from_numpy


# ------------------------------------------------------------------ one truth: the references against torch and the oracle
@pytest.mark.parametrize("shape", GB.POOL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pool_reference_and_emulation_are_torchs(shape):
    """the emulation is torch's fp32 max_pool2d bit for bit, its taps are torch's first maximum, the float64 output rounded to
    fp32 is the same, the output size is torch's; the backward emulation meets the bound and the unit is what it says"""
    for fam in GB.POOL_FAMILIES:
        x, g = GB.pool_case(fam, shape)
        assert np.isfinite(x).all()
        y32, idx = F.max_pool2d(T(x), 3, 2, 1, ceil_mode=True, return_indices=True)
        assert y32.shape[2:] == (GB.pool_out(shape[2]), GB.pool_out(shape[3])) == g.shape[2:]
        y64, tap, dx64, unit = GB.pool_ref64(x, g)
        ye, te = GB.emu_pool_fwd(x)
        assert GB.bits_equal(ye, y32.numpy()) and GB.bits_equal(ye, y64.astype(f32)) and np.array_equal(te, tap), fam
        ho, wo = np.arange(tap.shape[2])[:, None], np.arange(tap.shape[3])[None, :]
        assert np.array_equal((ho * 2 - 1 + tap // 3) * shape[3] + (wo * 2 - 1 + tap % 3), idx.numpy())
        if fam != "normal" and shape[2] * shape[3] > 1:        # the family holds what it promises: windows with a repeated maximum
            assert not np.array_equal(GB.emu_pool_fwd(x, fault="ties_last_tap")[1], tap)
            assert (GB.emu_pool_fwd(x, fault="ties_last_tap")[1] != tap).mean() >= (0.3 if shape[2] > 2 else 0.05), fam
        # the unit: sum |g| over the windows whose tap names the pixel, at most four of them
        cnt = GB.pool_ref64(x, np.ones_like(g))[3]
        assert cnt.max() <= 4 and abs(unit.sum() - np.abs(g).astype(f64).sum()) <= 1e-9 * unit.sum()
        for got in (GB.emu_pool_bwd(g, te, shape[2], shape[3]), GB.torch_pool_bwd_fp32(x, g)):
            assert GB.rel_excess(got, dx64, GB.E_pool_bwd() * unit) <= 1.0, fam
        # all four windows of a pixel choose it somewhere from 4 x 3 on; all-equal images give every window a pixel of its own
        assert cnt.max() == (1 if fam == "equal" or shape[2] == 1 else 4 if fam == "normal" or shape[2] >= 4 else 2), (fam, cnt.max())


@pytest.mark.parametrize("lo,hi", GB.BILR_SHAPES)
def test_bilinear_rows_references(lo, hi):
    """forward: float64 is torch's float64 interpolate up to the float64 rounding of the fp32 coordinates, the emulation (the
    oracle's three-FMA expression) and torch fp32 are inside the bound; backward: the emulation of the kernel's own
    order and torch fp32 inside the bound"""
    for C in (4, 20):
        x, g = GB.bilr_case(lo, hi, 3 if C == 4 else 1, C)
        ref = GB.bilinear_fwd64(x, *hi)
        tor = F.interpolate(T(x).double(), hi, mode="bilinear", align_corners=True).numpy()
        unit = GB.bilr_fwd_unit(x, *hi)
        r1, u1 = GB.bilinear_bwd64(g, *lo)                              # the matrix-product forms are loss_bounds' einsums
        r2, u2 = GB.bilr_bwd64(g, *lo)
        assert np.abs(GB.bilr_fwd64(x, *hi) - ref).max() <= 1e-13 * unit.max() and np.abs(r1 - r2).max() <= 1e-13 * u1.max()
        assert np.abs(u1 - u2).max() <= 1e-13 * u1.max()
        # torch's float64 coordinates are not the forward's fp32 ones: a source coordinate carries two fp32 roundings (the scale,
        # the product) of a value below the input size, and moves the output by at most that times |v1 - v0| <= 2 max |x|
        assert np.abs(ref - tor).max() <= 4 * GB.EPS * (lo[0] + lo[1]) * np.abs(x).max()
        emu = GB.emu_bilr_fwd(x, *hi)
        for got in (emu, GB.torch_bilr_fwd_fp32(x, *hi)):              # (torch's vectorised CPU path has its own operation order)
            assert GB.rel_excess(got, ref, GB.E_bilr_fwd() * unit) <= 1.0
        assert GB.bilr_bwd_excess(GB.emu_bilr_bwd(g, *lo), g, *lo) <= 1.0
        assert GB.bilr_bwd_excess(GB.torch_bilinear_bwd_fp32(g, *lo), g, *lo) <= 1.0
    Ay, Ax = GB.ac_matrix(hi[0], lo[0]), GB.ac_matrix(hi[1], lo[1])
    ky, kx = int((Ay != 0).sum(0).max()), int((Ax != 0).sum(0).max())
    assert GB.bilr_bwd_count(Ay, Ax) == ky * kx + 3 and ky >= 1 and kx >= 1


def test_row_copy_broadcast_references_are_exact():
    for M in GB.ROW_M:
        for C in GB.ROW_C:
            s, d = GB.rows_case(M, C), GB.rows_case(M, C, tag=1)
            for acc in (0, 1):
                assert GB.bits_equal(GB.copy_rows_ref(s, d, acc), GB.emu_copy_rows(s, d, acc))
            for scale in GB.BCAST_SCALES:
                for rpi in GB.BCAST_RPI:
                    v = GB.rows_case(-(-M // rpi), C, tag=2)
                    a, b = GB.broadcast_ref(v, scale, rpi, M), GB.emu_broadcast(v, scale, rpi, M)
                    assert GB.bits_equal(a, b) and a.shape == (M, C)
                    assert GB.bits_equal(a, (T(v)[torch.arange(M) // rpi] * float(f32(scale))).numpy())


@pytest.mark.parametrize("shape", GB.GAP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gap_references(shape):
    x, g = GB.gap_case(shape)
    HW = shape[2] * shape[3]
    xt = T(x).double().requires_grad_(True)
    y = F.adaptive_avg_pool2d(xt, 1)
    y.backward(T(g).double()[:, :, None, None])
    ref = x.astype(f64).mean((2, 3))
    assert np.abs(ref - y.detach().numpy()[:, :, 0, 0]).max() <= 1e-14 * max(1.0, np.abs(ref).max())
    assert np.abs(xt.grad.numpy() - (g.astype(f64) / HW)[:, :, None, None]).max() <= 1e-15
    unit = np.abs(x.astype(f64)).mean((2, 3))
    for got in (GB.emu_colsum(x, 1.0 / HW), F.adaptive_avg_pool2d(T(x), 1).numpy()[:, :, 0, 0]):
        assert GB.rel_excess(got, ref, GB.E_gap_fwd(HW) * unit) <= 1.0
    for got in (GB.emu_colsum(x, 1.0), T(x).sum((2, 3)).numpy()):
        assert GB.rel_excess(got, x.astype(f64).sum((2, 3)), GB.E_colsum(HW) * unit * HW) <= 1.0
    gb = GB.emu_broadcast(g, 1.0 / HW, 1, shape[0])
    assert GB.rel_excess(gb, g.astype(f64) / HW, GB.E_gap_bwd() * np.abs(g.astype(f64)) / HW) <= 1.0
    assert GB.colsum_rows_per_block(64 * 512 + 1) == (65, 512) and GB.colsum_rows_per_block(1) == (1, 1)


@pytest.mark.parametrize("C", GB.SOFTMAX_C)
def test_softmax_rows_reference_emulation_and_torch(C):
    for fam in GB.SOFTMAX_FAMILIES:
        for M in GB.SOFTMAX_M:
            z = GB.softmax_case(fam, C, M)
            assert z.shape == (M, C) and np.isfinite(z).all()
            ref = GB.softmax_ref64(z)
            assert np.abs(ref - F.softmax(T(z).double(), 1).numpy()).max() <= 1e-15
            for got in (GB.emu_softmax_rows(z), F.softmax(T(z), 1).numpy(), R.softmax_nchw(z.T[None, :, :, None])[0, :, :, 0].T):
                assert max(GB.softmax_excess(got, z)) <= 1.0, (fam, M)


def test_dense_small_reference_and_bound():
    for fam in GB.DENSE_FAMILIES:
        for M, K, Cout in ((1, 4, 1), (5, 252, 3), (16, 2048, 6), (2, 260, 256)):
            x, w, b = GB.dense_case(fam, M, K, Cout)
            for bias in (b, None):
                y, _ = GB.dense_ref64(x, w, bias)
                assert np.abs(y - F.linear(T(x).double(), T(w).double(), None if bias is None else T(bias).double()).numpy()).max() <= 1e-12
                assert GB.dense_excess(GB.emu_dense(x, w, bias), x, w, bias) <= 1.0
    x, w, b = GB.dense_case("pooled", 16, 2048, 6)
    assert np.abs(x / x[:1] - 1).max() < 0.1                                        # rows that differ by about 1 %
    assert GB.dense_excess(F.linear(T(x), T(w), T(b)).numpy(), x, w, b) > 1.0       # an fp32 dot product is NOT inside this bound


@pytest.mark.parametrize("n", GB.OPT_N)
def test_sgd_emulation_is_the_oracles_and_inside_the_float64_bound(n):
    p, grads = GB.opt_case(n, GB.SGD_STEPS)
    for b1, b2 in GB.seg_table(n):
        lr = GB.seg_lr(n, b1, b2, GB.SGD_LRS)
        assert (lr[:b1] == f32(GB.SGD_LRS[0])).all() and (lr[b1:b2] == f32(GB.SGD_LRS[1])).all() and (lr[b2:] == f32(GB.SGD_LRS[2])).all()
        for gs in GB.SGD_SCALES:
            for wd in GB.SGD_DECAYS:
                a = (p, grads, b1, b2, GB.SGD_LRS, GB.SGD_MOMENTUM, wd, gs)
                emu, ref = GB.emu_sgd(*a), GB.sgd_ref64(*a)
                cur, buf = p.copy(), np.zeros_like(p)          # the oracle, segment by segment
                for k, g in enumerate(grads):
                    nc, nb = np.empty_like(p), np.empty_like(p)
                    for lo, hi, l in ((0, b1, GB.SGD_LRS[0]), (b1, b2, GB.SGD_LRS[1]), (b2, n, GB.SGD_LRS[2])):
                        nc[lo:hi], nb[lo:hi] = R.sgd_step(cur[lo:hi], (g[lo:hi] * f32(gs)).astype(f32), buf[lo:hi], l, GB.SGD_MOMENTUM, wd, k == 0)
                    cur, buf = nc, nb
                    assert GB.bits_equal(emu[k][0], cur) and GB.bits_equal(emu[k][1], buf)
                assert GB.sgd_excess(emu, ref) <= 1.0 and GB.sgd_excess(GB.torch_sgd_fp32(*a), ref) <= 1.0


@pytest.mark.parametrize("betas", GB.ADAM_BETAS, ids=lambda b: f"beta2_{b[1]}")
def test_adam_emulation_and_torch_fp32_inside_the_bounds(betas):
    for n in GB.OPT_N:
        p, grads = GB.opt_case(n, GB.ADAM_STEPS)
        for b1, b2 in GB.seg_table(n):
            a = (p, grads, b1, b2, GB.ADAM_LRS, betas, GB.ADAM_EPS)
            ref = GB.adam_ref64(*a)
            lr = GB.seg_lr(n, b1, b2, GB.ADAM_LRS).astype(f64)
            for got in (GB.emu_adam(*a), GB.torch_adam_fp32(*a)):
                ex = GB.adam_excess(got, ref, p, grads, lr, betas)
                assert max(ex.values()) <= 1.0, (n, b1, b2, ex)
    om = GB.adam_host_args(betas, 1)
    assert f32(om[1]) == f32(1.0 - betas[0]) and f32(om[3]) == f32(1.0 - betas[1])


def test_ema_emulation_is_the_oracles_and_inside_the_float64_bound():
    t, (s,) = GB.opt_case(1000, 1, seed=3)
    for d in GB.EMA_DECAYS:
        emu = GB.emu_ema(t, s, d)
        assert GB.bits_equal(emu, R.ema_update(t, s, d))
        ref, unit = GB.ema_ref64(t, s, d)
        assert GB.rel_excess(emu, ref, GB.E_ema() * unit + 1e-300) <= 1.0
        if d == 0.0:
            assert GB.bits_equal(emu, s)


def test_mix_references_are_the_oracles():
    for B in GB.MIX_B:
        for C in GB.MIX_C:
            for H, W in GB.MIX_HW:
                img, lab, conf = GB.mix_case(B, C, H, W)
                assert set(np.unique(lab)) <= set(GB.MIX_LABELS) and (H * W * B < 9 or {63, 64, 255} <= set(np.unique(lab)))
                for boxes in GB.mix_boxes(B, H, W):
                    assert all(0 <= y0 <= y1 <= H and 0 <= x0 <= x1 <= W for y0, y1, x0, x1 in boxes)
                    for mode, orc in (("cutmix", R.cutmix_apply), ("cutout", R.cutout_apply)):
                        a, b = GB.mix_ref(mode, img, lab, conf, boxes=boxes), orc(img, lab, conf, boxes)
                        assert all(GB.bits_equal(u, v) for u, v in zip(a, b)), (mode, boxes)
                for sel in GB.mix_selections(B):
                    chosen = [[c for c in range(64) if (int(w) >> c) & 1] for w in sel]
                    a, b = GB.mix_ref("classmix", img, lab, conf, sel=sel), R.classmix_apply(img, lab, conf, chosen)
                    assert all(GB.bits_equal(u, v) for u, v in zip(a, b))
    kinds = GB.mix_boxes(1, 33, 35)
    assert kinds[0][0][0] == kinds[0][0][1] and kinds[1][0] == (0, 33, 0, 35) and kinds[2][0] == (0, 1, 0, 1) and kinds[3][0][1::2] == (33, 35)


def test_presence_and_window_references():
    for HW in GB.PRESENCE_HW:
        lab = GB.presence_case(5, HW)
        bits = GB.presence_ref(lab)
        for i in range(5):
            want = sum(1 << int(v) for v in set(lab[i].tolist()) if 0 <= v < 64)
            assert int(bits[i]) == want
        if HW >= 255:
            assert all((lab[i] == lab[i, -1]).sum() == 1 for i in range(5))
    assert {int(b) for b in GB.presence_ref(GB.presence_case(4, 257))} >= {1, 1 << 63, (1 << 63) | 1}
    for C in GB.WIN_C:
        srcs = GB.window_case(C)
        pred, count = GB.emu_windows(C, srcs)
        assert count.min() >= 1 and count.max() >= 3 and all(w[0] + w[2] <= 9 and w[1] + w[3] <= 11 for w in GB.WINDOWS)
        p64 = np.zeros(pred.shape)
        for (h0, w0, hc, wc), s in zip(GB.WINDOWS, srcs):
            p64[:, h0:h0 + hc, w0:w0 + wc] += s
        assert np.abs(pred - p64).max() <= 6 * GB.EPS * np.abs(p64).max() + 1e-6


# ------------------------------------------------------------------ the calibrated ceilings, re-measured
def test_ceilings_are_what_torch_fp32_reaches():
    """every CAL_* constant is a ceiling of what torch's fp32 arithmetic reaches against float64, and not more than twice it"""
    tor, emu = {}, {}
    for form, out in (("torch", tor), ("emu", emu)):
        out["CAL_POOL_BWD"] = GB.measure_pool_bwd(form)
        out["CAL_BILR_FWD"], out["CAL_BILR_BWD"] = GB.measure_bilr(form)
        out["CAL_GAP_FWD"], out["CAL_GAP_BWD"], out["CAL_COLSUM"] = GB.measure_gap(form)
        out["CAL_SGD"] = GB.measure_sgd(form)
        ad = [GB.measure_adam(b, form) for b in GB.ADAM_BETAS]
        out["CAL_ADAM_V"], out["CAL_ADAM_M"], out["CAL_ADAM_U"] = (tuple(a[k] for a in ad) for k in ("exp_avg_sq", "exp_avg", "update"))
        out["CAL_EMA"] = GB.measure_ema(form)
    print()
    for k in tor:
        fmt = lambda v: " ".join(f"{x:.2f}" for x in (v if isinstance(v, tuple) else (v,)))
        print(f"  {k:14s} = {getattr(GB, k):<5}  torch fp32 {fmt(tor[k])}   [emulation {fmt(emu[k])}]")
        m = max(tor[k]) if isinstance(tor[k], tuple) else tor[k]
        assert m <= getattr(GB, k) <= 2 * m, (k, m)
    bad = [GB.measure_adam(b, "emu", fault="fp32_one_minus_beta")["exp_avg_sq"] for b in GB.ADAM_BETAS]
    print("  exp_avg_sq with 1.0f - beta2 formed on the device: " + " ".join(f"{v:.1f}" for v in bad))


# ------------------------------------------------------------------ the bounds reject faulty arithmetic
def test_fault_pool_last_partial_window_dropped():
    """even image sizes end in a partial window: (2, 64, 34, 36), family normal"""
    x, _ = GB.pool_case("normal", (2, 64, 34, 36))
    y64, tap = GB.pool_ref64(x)
    y, t = GB.emu_pool_fwd(x, fault="drop_last_window")
    assert not GB.bits_equal(y, y64.astype(f32)) and not np.array_equal(t, tap)
    assert GB.bits_equal(y[:, :, :17, :18], y64.astype(f32)[:, :, :17, :18])       # only the last window of each axis differs
    x, _ = GB.pool_case("normal", (2, 64, 33, 35))                                 # an odd size has no partial window
    assert GB.bits_equal(GB.emu_pool_fwd(x, fault="drop_last_window")[0], GB.pool_ref64(x)[0].astype(f32))


def test_fault_pool_ties_to_the_last_tap():
    """family ties at (2, 8, 3, 4): the output is unchanged, the taps are not, and the backward leaves its bound"""
    shape = (2, 8, 3, 4)
    x, g = GB.pool_case("ties", shape)
    y64, tap, dx64, unit = GB.pool_ref64(x, g)
    y, t = GB.emu_pool_fwd(x, fault="ties_last_tap")
    assert GB.bits_equal(y, y64.astype(f32)) and not np.array_equal(t, tap)
    bound = GB.E_pool_bwd() * unit
    assert not GB.rel_excess(GB.emu_pool_bwd(g, t, 3, 4), dx64, bound) <= 1.0
    x, g = GB.pool_case("normal", shape)                                           # without ties the fault is invisible
    assert np.array_equal(GB.emu_pool_fwd(x, fault="ties_last_tap")[1], GB.pool_ref64(x)[1])


def test_fault_bilinear_backward_skips_coinciding_taps():
    """(5, 7) -> (17, 23): the last output row and column have i1 == i0; (1, 5) -> (4, 5): every row has"""
    for lo, hi in (((5, 7), (17, 23)), ((1, 5), (4, 5))):
        _, g = GB.bilr_case(lo, hi, 1, 4)
        assert GB.bilr_bwd_excess(GB.emu_bilr_bwd(g, *lo), g, *lo) <= 1.0
        assert GB.bilr_bwd_excess(GB.emu_bilr_bwd(g, *lo, fault="skip_i1_eq_i0"), g, *lo) > 1e3


def test_fault_sgd_segment_boundary_off_by_one():
    """n = 1000, (b1, b2) = (77, 301): elements 77 and 301 take their neighbour's learning rate"""
    n, b1, b2 = 1000, 77, 301
    p, grads = GB.opt_case(n, GB.SGD_STEPS)
    a = (p, grads, b1, b2, GB.SGD_LRS, GB.SGD_MOMENTUM, 5e-4, 1.0 / 3)
    ref, bad = GB.sgd_ref64(*a), GB.emu_sgd(*a, fault="segment_off_by_one")
    assert GB.sgd_excess(bad, ref) > 1e3
    diff = np.flatnonzero(bad[0][0] != GB.emu_sgd(*a)[0][0])
    assert set(diff) <= {b1, b2} and len(diff) >= 1
    assert GB.sgd_excess(GB.emu_sgd(*a), ref) <= 1.0


def test_fault_adam_one_minus_beta2_formed_in_fp32():
    """the kernel before the fix at beta2 = 0.999, n = 1000, (b1, b2) = (77, 301): exp_avg_sq is the quantity out of bound (about
    219 units against a bound of at most 18), exp_avg is not; with the host-formed weights all three are inside"""
    betas, n, b1, b2 = (0.9, 0.999), 1000, 77, 301
    assert float(f32(1) - f32(0.999)) != float(f32(0.001)) and abs(float(f32(1) - f32(0.999)) - 0.0009999871) < 1e-10
    p, grads = GB.opt_case(n, GB.ADAM_STEPS)
    a = (p, grads, b1, b2, GB.ADAM_LRS, betas, GB.ADAM_EPS)
    ref, lr = GB.adam_ref64(*a), GB.seg_lr(n, b1, b2, GB.ADAM_LRS).astype(f64)
    bad = GB.adam_excess(GB.emu_adam(*a, fault="fp32_one_minus_beta"), ref, p, grads, lr, betas)
    good = GB.adam_excess(GB.emu_adam(*a), ref, p, grads, lr, betas)
    print(f"\n  fp32 1 - beta: {bad}\n  host 1 - beta: {good}", end="")
    assert bad["exp_avg_sq"] > 10.0 and bad["exp_avg"] <= 1.0, bad
    assert max(good.values()) <= 1.0, good
    worst = GB.measure_adam(betas, "emu", fault="fp32_one_minus_beta")["exp_avg_sq"]
    assert 200 < worst < 240, worst


def test_fault_box_includes_its_end_row():
    """B = 2, C = 3, 5 x 7, the one-pixel corner box and the box that ends inside the image"""
    img, lab, conf = GB.mix_case(2, 3, 5, 7)
    boxes = [(0, 1, 0, 1), (1, 3, 2, 5)]
    for mode in ("cutmix", "cutout"):
        good, bad = GB.mix_ref(mode, img, lab, conf, boxes=boxes), GB.mix_ref(mode, img, lab, conf, boxes=boxes, fault="box_includes_end_row")
        assert not GB.bits_equal(good[0], bad[0]) and not GB.bits_equal(good[2], bad[2])
        assert GB.bits_equal(good[0][:, :, 4:], bad[0][:, :, 4:])


def test_fault_classmix_label_cast_before_the_blend():
    """labels of 128 and above (254, 255) do not survive an 8-bit cast: B = 2, 33 x 35, any selection"""
    img, lab, conf = GB.mix_case(2, 1, 33, 35)
    sel = GB.mix_selections(2)[0]
    good, bad = GB.mix_ref("classmix", img, lab, conf, sel=sel), GB.mix_ref("classmix", img, lab, conf, sel=sel, fault="label_cast_int8_before_blend")
    assert not np.array_equal(good[1], bad[1]) and (good[1] == 255).any() and GB.bits_equal(good[0], bad[0])
    assert set(np.unique(good[1])) <= set(GB.MIX_LABELS)
    assert math.isfinite(float(good[2].sum()))
