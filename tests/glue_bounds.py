"""Float64 references, numpy fp32 emulations, input families, shape tables and error bounds of the "glue" kernels in the second
half of u2pl_amd/csrc/nn.hip, shared by the CPU file (tests/test_glue_bounds_cpu.py) and the GPU file
(tests/test_gpu_glue_bounds.py).  Not a conftest: imported by name, like loss_bounds.

Covered: k_maxpool_fwd / k_maxpool_bwd, k_bilinear_rows_fwd / k_bilinear_rows_bwd, k_copy_rows, k_copy_cols, k_broadcast_rows,
the global average pool (k_colreduce_partial + k_colreduce_final + k_sums_to_f32), k_softmax_rows, k_dense_small, k_sgd, k_adam,
k_ema, k_cutmix, k_strong_aug, k_label_presence, k_window_acc, k_window_div.  Every reference starts from the fp32 ARGUMENTS of
the kernel (a kernel's contract begins there: a learning rate, a decay or a scale is the float the host hands over).

EXACT operations (maximum and its tap, copies, the broadcast's one product, the one-add accumulate, the box mixes, label presence,
the window adds) are asserted bit for bit against the numpy fp32 emulation AND against the float64 reference rounded to fp32.

Every other element is held to  |got - ref64| <= EPS min(derived, CAL_MARGIN measured) unit  where `derived` is the first-order
rounding count of the kernel's own order (the *_count functions: one unit per fp32 rounding), `measured` the ceiling that THE
REFERENCE'S OWN fp32 ARITHMETIC (torch on the CPU) reaches against float64 over the families and shapes of the tables below --
never a HIP kernel -- and `unit` the sum of absolute terms named beside each count.  Measured (python -m pytest
tests/test_glue_bounds_cpu.py -s -k ceilings; the emulation of the kernels' order in brackets):

    pool backward      units of EPS sum |g| over the windows that chose the pixel, POOL_SHAPES x POOL_FAMILIES:      2.35 [2.35]
    bilinear forward   units of EPS |A_y| |x| |A_x|, BILR_SHAPES:                                                    2.83 [2.40]
    bilinear backward  units of EPS |A_y|^T |g| |A_x|, BILR_SHAPES (loss_bounds.measure_bilinear):                   2.80 [3.18]
    average pool fwd   units of EPS mean |x|, GAP_SHAPES:                                                            1.62 [2.94]
    average pool bwd   units of EPS |g| / HW:                                                                        0.94 [1.40]
    column sums        units of EPS sum |g| (backward of the 1x1 broadcast), GAP_SHAPES:                             1.59 [2.67]
    SGD                units of EPS sum_s (t - s + 1) unit_s, three steps, seg_table x the scale / decay grid:       1.16 [1.38]
    Adam exp_avg_sq    units of EPS v, five steps:             beta2 = 0.99: 3.35 [3.50]    beta2 = 0.999: 4.38 [4.10]
    Adam exp_avg       units of EPS max_s |g_s|:                             0.40 [0.43]                   0.40 [0.43]
    Adam update        units of EPS lr beyond the rounding EPS |p_t| of the stored parameter:  3.27 [1.65]  1.81 [2.07]
    EMA                units of EPS (|d t| + |(1 - d) s|):                                                           1.80 [1.80]
    softmax_rows       loss_bounds.E_prob (its own table)

(EPS = 2^-24 is the largest RELATIVE error of one rounding, so every rounding counts one unit, the rounding of a constant such as
float32(1 / HW) or float32(1 - beta2) included.)

FINDING 1 (fixed with this suite): k_adam formed `1.0f - beta2` in fp32 on the device; torch forms 1 - beta2 in double and rounds
once.  At beta2 = 0.999 the device weight was 0.0009999871 instead of float32(0.001), and the emulation of that order leaves
exp_avg_sq 219 units from torch's float64 Adam after five steps (torch's own fp32 Adam 4.4, the emulation with host-formed weights
4.1; at beta2 = 0.99: 18.5 units).  u2pl_adam_step_f32 now takes one_minus_beta1 / one_minus_beta2 from the host, as
u2pl_ema_update_f32 takes one_minus_decay; emu_adam(fault="fp32_one_minus_beta") keeps the old order and
tests/test_glue_bounds_cpu.py shows that adam_excess names exp_avg_sq for it.
FINDING 2: "the parameter update p_t - p_{t-1} relative to lr" cannot be resolved below the rounding of the stored fp32 parameter
itself: p_t = rn(p_{t-1} - u) carries EPS |p_t|, which at |p| = 1 and lr = 1e-3 is 1000 units of EPS lr (torch's own fp32 Adam
is hundreds of them off on opt_case inputs).  The bound is therefore EPS (|p_t| + min(count, CAL_MARGIN measured) lr): one rounding of the
stored value, the update relative to lr.
FINDING 3 (fixed with this suite): u2pl_maxpool3s2_bwd_f32 had no C % 4 guard and would have skipped the last C % 4 channels
silently; it now returns 1001 like the forward.
FINDING 4: on the device exp_avg and exp_avg_sq of k_adam are emu_adam's bit for bit (products and sums only; asserted), the
parameter is not (printed, not asserted): the square root and the divisions behind the update are not all IEEE-rounded on the
device whatever their _rn names say.  The difference stays inside the update's bound (largest observed 0.98 of it, most of which
is the rounding EPS |p_t| of the stored parameter, FINDING 2).

No infinities or NaN anywhere, every label, index, box and window inside its contract; no case launches an out-of-contract shape
(the argument-contract test only calls entry points that return 1001 BEFORE any launch)."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from contrast_bounds import CAL_MARGIN  # noqa: F401  (one definition for all bound modules)
from loss_bounds import (BIL_SHAPES, CLASSES, E_prob, ac_coord, ac_matrix, bilinear_bwd64, bilinear_fwd64,  # noqa: F401
                         make_case, measure_bilinear, s_count, torch_bilinear_bwd_fp32)
from split_bounds import EPS

f32 = np.float32
f64 = np.float64
SENTINEL_BITS = 0x7149F2CA          # float32 1.0e30: finite, and no kernel of this file produces it
GRID_CAP = 4096 * 256               # grid_for(): 4096 blocks of 256 threads; one work item more takes a second trip

# ---- calibrated ceilings: torch's own fp32 arithmetic against float64 (never the HIP kernels); table in the module docstring.
# Each is the measured value rounded up by a few per cent (torch's reduction order may differ between CPUs), never to more than twice it
CAL_POOL_BWD = 2.5       # measured 2.35: the <= 4 gradients of a pixel added in fp32
CAL_BILR_FWD = 3.0       # measured 2.83
CAL_BILR_BWD = 2.9       # measured 2.80 (loss_bounds.CAL_BIL over BIL_SHAPES; the three extra shapes stay below it)
CAL_GAP_FWD = 2.0        # measured 1.62
CAL_GAP_BWD = 1.0        # measured 0.94
CAL_COLSUM = 2.0         # measured 1.59
CAL_SGD = 1.4            # measured 1.16
CAL_ADAM_V = 4.6         # measured 3.35 (beta2 = 0.99) 4.38 (0.999)
CAL_ADAM_M = 0.45        # measured 0.40
CAL_ADAM_U = 3.5         # measured 3.27 1.81
CAL_EMA = 2.0            # measured 1.80


def _b(derived, cal):
    """the asserted count: the derived one and CAL_MARGIN times the measured ceiling, the smaller"""
    return min(derived, CAL_MARGIN * cal)


def rel_excess(got, ref, bound):
    """max |got - ref| / bound over all elements (inf where got is not finite); elements with a zero bound must be equal"""
    got, ref, bound = np.asarray(got, dtype=f64), np.asarray(ref, dtype=f64), np.asarray(bound, dtype=f64)
    if not np.isfinite(got).all():
        return math.inf
    d = np.abs(got - ref)
    if ((bound == 0) & (d != 0)).any():
        return math.inf
    return float((d / np.where(bound == 0, 1.0, bound)).max()) if d.size else 0.0


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# =================================================================== max pool 3x3, stride 2, padding 1, ceil_mode ================
POOL_SHAPES = ((1, 4, 1, 1), (1, 4, 2, 2), (2, 8, 3, 4), (2, 8, 4, 3), (1, 12, 7, 10), (2, 64, 33, 35), (2, 64, 34, 36))
POOL_FAMILIES = ("normal", "ties", "equal")
POOL_STRIDE_SHAPE = (2, 128, 257, 257)      # forward 2 x 129 x 129 x 32 and backward 2 x 257 x 257 x 32 float4 items > 2^20
POOL_FAULTS = ("drop_last_window", "ties_last_tap")


def pool_out(n):
    """torch's ceil_mode output size for (3, 2, 1): the last window must start inside the image or its left padding"""
    o = -(-(n + 2 - 3) // 2) + 1
    return o - 1 if (o - 1) * 2 >= n + 1 else o


def pool_case(family, shape, seed=0):
    """x [N, C, H, W] and the upstream gradient g [N, C, Ho, Wo], float32.  ties: a grid of 1/4 in [-1/2, 1/2] (five values), so that
    windows hold their maximum more than once; equal: one value everywhere, every window tied in all its taps"""
    N, C, H, W = shape
    rng = np.random.default_rng([seed, 11, POOL_FAMILIES.index(family), N, C, H, W])
    x = rng.standard_normal(shape, dtype=f32)
    if family == "ties":
        x = (np.round(np.clip(x, -0.5, 0.5) * f32(4)) / f32(4)).astype(f32)
    elif family == "equal":
        x = np.full(shape, f32(-1.75))
    g = rng.standard_normal((N, C, pool_out(H), pool_out(W)), dtype=f32)
    return np.ascontiguousarray(x, dtype=f32), g


def pool_ref64(x, g=None):
    """F.max_pool2d(3, 2, 1, ceil_mode=True) in float64 -> y [N, C, Ho, Wo], tap uint8 (r * 3 + s of torch's index: the FIRST
    maximum in row-major order); with g also the float64 autograd gradient and the bound's unit, sum |g| over the windows
    that chose the pixel"""
    xt = torch.from_numpy(np.ascontiguousarray(x)).double().requires_grad_(g is not None)
    y, idx = F.max_pool2d(xt, 3, 2, 1, ceil_mode=True, return_indices=True)
    H, W = x.shape[2:]
    ih, iw = (idx // W).numpy(), (idx % W).numpy()
    ho = np.arange(y.shape[2])[:, None]
    wo = np.arange(y.shape[3])[None, :]
    tap = ((ih - (ho * 2 - 1)) * 3 + (iw - (wo * 2 - 1))).astype(np.uint8)
    if g is None:
        return y.detach().numpy(), tap
    gt = torch.from_numpy(np.ascontiguousarray(g)).double()
    (dx,) = torch.autograd.grad(y, xt, gt, retain_graph=True)
    (unit,) = torch.autograd.grad(y, xt, gt.abs())
    return y.detach().numpy(), tap, dx.numpy(), unit.numpy()


def emu_pool_fwd(x, fault=None):
    """k_maxpool_fwd: the nine taps in row-major order, the first in-image tap taken unconditionally, then strictly greater.
    drop_last_window: the output size of floor mode, the last partial window is never written (0, tap 0);
    ties_last_tap: >= instead of >"""
    N, C, H, W = x.shape
    Ho, Wo = pool_out(H), pool_out(W)
    best = np.full((N, C, Ho, Wo), -np.inf, dtype=f32)
    tap = np.zeros((N, C, Ho, Wo), dtype=np.uint8)
    seen = np.zeros((Ho, Wo), dtype=bool)
    for r in range(3):
        ih = np.arange(Ho) * 2 - 1 + r
        vy = (ih >= 0) & (ih < H)
        for s in range(3):
            iw = np.arange(Wo) * 2 - 1 + s
            valid = vy[:, None] & ((iw >= 0) & (iw < W))[None, :]
            v = x[:, :, np.clip(ih, 0, H - 1)][:, :, :, np.clip(iw, 0, W - 1)]
            upd = valid & (~seen | ((v >= best) if fault == "ties_last_tap" else (v > best)))
            best = np.where(upd, v, best)
            tap = np.where(upd, np.uint8(r * 3 + s), tap)
            seen = seen | valid
    if fault == "drop_last_window":
        fo_h, fo_w = (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1
        best[:, :, fo_h:], best[:, :, :, fo_w:], tap[:, :, fo_h:], tap[:, :, :, fo_w:] = 0, 0, 0, 0
    return best, tap


def emu_pool_bwd(g, tap, H, W):
    """k_maxpool_bwd: every input pixel adds the gradients of the <= 4 windows whose tap names it, ho ascending, then wo ascending
    (larger ho is the smaller r), in fp32"""
    N, C, Ho, Wo = g.shape
    dx = np.zeros((N, C, H, W), dtype=f32)
    for r in (2, 1, 0):
        ih = np.arange(Ho) * 2 - 1 + r
        for s in (2, 1, 0):
            iw = np.arange(Wo) * 2 - 1 + s
            ok = ((ih >= 0) & (ih < H))[:, None] & ((iw >= 0) & (iw < W))[None, :]
            hit = (tap == r * 3 + s) & ok
            n, c, ho, wo = np.nonzero(hit)
            dx[n, c, ih[ho], iw[wo]] = (dx[n, c, ih[ho], iw[wo]] + g[n, c, ho, wo]).astype(f32)     # one window per pixel and tap
    return dx


def torch_pool_bwd_fp32(x, g):
    xt = torch.from_numpy(np.ascontiguousarray(x)).requires_grad_(True)
    F.max_pool2d(xt, 3, 2, 1, ceil_mode=True).backward(torch.from_numpy(np.ascontiguousarray(g)))
    return xt.grad.numpy()


POOL_BWD_COUNT = 3      # a pixel lies in at most four windows: three fp32 adds (the first lands on 0)


def E_pool_bwd():
    """in units of sum |g| over the windows that chose the pixel"""
    return EPS * _b(POOL_BWD_COUNT, CAL_POOL_BWD)


# =================================================================== bilinear rows (align_corners=True feature maps) ============
BILR_SHAPES = BIL_SHAPES + (((1, 5), (4, 5)), ((5, 1), (5, 7)), ((5, 7), (1, 1)))        # (input, output)
BILR_C = (4, 20, 256)
BILR_N = (1, 3)
BILR_STRIDE_FWD = ((1, 64), (129, 129), (257, 257))     # 257 * 257 * 16 float4 items
BILR_STRIDE_BWD = ((1, 64), (257, 257), (300, 300))     # items of the BACKWARD: one per input element, 257 * 257 * 16


def bilr_case(lo, hi, N, C, seed=0):
    """x [N, C, h, w] and the upstream gradient g [N, C, H, W], float32"""
    rng = np.random.default_rng([seed, 12, lo[0], lo[1], hi[0], hi[1], N, C])
    return rng.standard_normal((N, C) + tuple(lo), dtype=f32), rng.standard_normal((N, C) + tuple(hi), dtype=f32)


def bilr_fwd64(x, H, W, absolute=False):
    """loss_bounds.bilinear_fwd64 (out = A_y x A_x^T) as two matrix products, for the 256-channel and the grid-stride cases;
    absolute: |A_y| |x| |A_x|^T, the unit of the forward's bound.  tests/test_glue_bounds_cpu.py pins it to the einsum"""
    x = np.asarray(x, dtype=f64)
    Ay, Ax = ac_matrix(H, x.shape[2]), ac_matrix(W, x.shape[3])
    if absolute:
        x, Ay, Ax = np.abs(x), np.abs(Ay), np.abs(Ax)
    return np.matmul(np.matmul(Ay, x), Ax.T)


def bilr_fwd_unit(x, H, W):
    return bilr_fwd64(x, H, W, absolute=True)


def bilr_bwd64(g, h, w):
    """loss_bounds.bilinear_bwd64 as two matrix products -> gin = A_y^T g A_x and the unit |A_y|^T |g| |A_x|"""
    g = np.asarray(g, dtype=f64)
    Ay, Ax = ac_matrix(g.shape[2], h), ac_matrix(g.shape[3], w)
    return np.matmul(np.matmul(Ay.T, g), Ax), np.matmul(np.matmul(np.abs(Ay).T, np.abs(g)), np.abs(Ax))


BILR_FWD_COUNT = 4      # cx.l1 * v (1), the inner fma (1), cy.l1 * bottom (1), the outer fma (1): the bottom row carries all four


def E_bilr_fwd():
    """k_bilinear_rows_fwd in units of |A_y| |x| |A_x| (the matrices hold the forward's own fp32 weights, so those are exact)"""
    return EPS * _b(BILR_FWD_COUNT, CAL_BILR_FWD)


def bilr_bwd_count(Ay, Ax):
    """k_bilinear_rows_bwd, its own order: wy = l0 + l1 where both taps hit (1), the same for wx (1), ww = wy * wx (1), ww * g
    (1), and the ky kx - 1 sequential adds of the window (k = most outputs that read one input along an axis), in units of
    |A_y|^T |g| |A_x|.  (Not loss_bounds.bil_count: k_bilinear_up_bwd sums a row first and multiplies by wy afterwards.)"""
    return 4 + int((Ay != 0).sum(0).max()) * int((Ax != 0).sum(0).max()) - 1


def E_bilr_bwd(Ay, Ax):
    return EPS * _b(bilr_bwd_count(Ay, Ax), CAL_BILR_BWD)


def bilr_bwd_excess(got, g, h, w, ref_unit=None):
    ref, unit = ref_unit if ref_unit is not None else bilr_bwd64(g, h, w)
    return rel_excess(got, ref, E_bilr_bwd(ac_matrix(g.shape[2], h), ac_matrix(g.shape[3], w)) * unit)


def emu_bilr_fwd(x, H, W):
    """the three-FMA expression of k_bilinear_rows_fwd is oracle.restate.bilinear_ac's (oracle/restate.c, exact fmaf)"""
    from oracle import restate as R
    return R.bilinear_ac(x, H, W)


def emu_bilr_bwd(g, h, w, fault=None):
    """k_bilinear_rows_bwd: per input element, oy ascending, inside a row ox ascending, ww = wy * wx, acc += ww * g, all fp32
    (the library is built with -ffp-contract=off: a product and an add).  skip_i1_eq_i0: outputs whose two taps coincide
    contribute nothing"""
    g = np.asarray(g, dtype=f32)
    N, C, H, W = g.shape
    taps = []
    for n_out, n_in in ((H, h), (W, w)):
        i0, i1, l0, l1 = ac_coord(n_out, n_in)
        per = []
        for i in range(n_in):
            o = np.flatnonzero((i0 == i) | (i1 == i))
            wgt = (np.where(i0[o] == i, l0[o], f32(0)) + np.where(i1[o] == i, l1[o], f32(0))).astype(f32)
            if fault == "skip_i1_eq_i0":
                keep = i0[o] != i1[o]
                o, wgt = o[keep], wgt[keep]
            per.append((o, wgt))
        taps.append(per)
    out = np.zeros((N, C, h, w), dtype=f32)
    for iy, (oys, wys) in enumerate(taps[0]):
        for ix, (oxs, wxs) in enumerate(taps[1]):
            acc = np.zeros((N, C), dtype=f32)
            for oy, wy in zip(oys, wys):
                for ox, wx in zip(oxs, wxs):
                    acc = (acc + (f32(wy * wx) * g[:, :, oy, ox]).astype(f32)).astype(f32)
            out[:, :, iy, ix] = acc
    return out


def torch_bilr_fwd_fp32(x, H, W):
    return F.interpolate(torch.from_numpy(np.ascontiguousarray(x)), (H, W), mode="bilinear", align_corners=True).numpy()


# =================================================================== row copies, broadcast, concat ===========================
ROW_M = (1, 7, 257)
ROW_C = (4, 20, 256)
COL_C = (1, 19, 21)
BCAST_SCALES = (1.0, 1.0 / 323)
BCAST_RPI = (1, 17)
CAT_CHANNELS = (4, 256, 20)
ROW_STRIDE_ITEMS = GRID_CAP + 259       # M * C / 4 of the row kernels' second trip


def rows_case(M, C, seed=0, tag=0):
    return np.random.default_rng([seed, 13, tag, M, C]).standard_normal((M, C), dtype=f32)


def copy_rows_ref(src, dst, accumulate):
    """exact: a copy, or ONE fp32 add src + dst (the float64 sum of two fp32 values rounded to fp32 is the same number)"""
    return (src.astype(f64) + dst.astype(f64)).astype(f32) if accumulate else src.copy()


def emu_copy_rows(src, dst, accumulate):
    return (src + dst).astype(f32) if accumulate else src.copy()


def broadcast_ref(v, scale, rows_per_image, M):
    """dst[r] = v[r // rows_per_image] * scale: one fp32 product (the float64 product of two fp32 values is exact, so its
    rounding to fp32 is that product); scale is the float the host passes"""
    idx = np.arange(M) // rows_per_image
    return (v[idx].astype(f64) * f64(f32(scale))).astype(f32)


def emu_broadcast(v, scale, rows_per_image, M):
    return (v[np.arange(M) // rows_per_image] * f32(scale)).astype(f32)


# =================================================================== global average pool / column sums ========================
GAP_SHAPES = ((2, 4, 1, 1), (3, 20, 5, 7), (2, 256, 17, 19))


def gap_case(shape, seed=0):
    rng = np.random.default_rng([seed, 14] + list(shape))
    return rng.standard_normal(shape, dtype=f32) + f32(0.5), rng.standard_normal(shape[:2], dtype=f32)


def colsum_rows_per_block(HW):
    """csrc/nn.hip colreduce_blocks(): min(512, ceil(HW / 64)) blocks per image, ceil(HW / blocks) rows each"""
    nblk = min(512, max(1, -(-HW // 64)))
    return -(-HW // nblk), nblk


def colsum_count(HW):
    """the fp32 part of the column sum: a block adds its rows in fp32 (at most rows - 1 sequential adds whatever the split into
    streams), the blocks are added in double; then ONE rounding of double(sum) * double(scale) to fp32: in units of sum |x|"""
    return (colsum_rows_per_block(HW)[0] - 1) + 1


def E_gap_fwd(HW):
    """in units of mean |x| = sum |x| / HW; the scale 1 / HW is the float the host passes (a unit of its own)"""
    return EPS * _b(colsum_count(HW) + 1, CAL_GAP_FWD)


def E_colsum(HW):
    """the backward of the 1x1 broadcast: column sums at scale 1, in units of sum |g|"""
    return EPS * _b(colsum_count(HW), CAL_COLSUM)


GAP_BWD_COUNT = 2       # g * float32(1 / HW): the rounding of the scale and of the product, in units of |g| / HW


def E_gap_bwd():
    return EPS * _b(GAP_BWD_COUNT, CAL_GAP_BWD)


def emu_colsum(x, scale):
    """x [N, C, H, W] -> [N, C]: rows of an image split over the blocks, each block's rows added in fp32 in the order of
    k_colreduce_partial for C / 4 <= 64 (tr = 256 / (C / 4) row groups, row g + rg + k tr to stream k % 4 while four fit, the
    rest to stream 0, (a + b) + (c + d), then the row groups in order), the blocks in double, one rounding"""
    N, C, H, W = x.shape
    HW = H * W
    rows = x.transpose(0, 2, 3, 1).reshape(N, HW, C)
    per, nblk = colsum_rows_per_block(HW)
    tc = min(64, C // 4)
    tr = 256 // tc
    tot = np.zeros((N, C), dtype=f64)
    for b in range(nblk):
        rb, re = b * per, min(HW, b * per + per)
        blk = np.zeros((N, C), dtype=f32)
        first = True
        for rg in range(tr):
            st = [np.zeros((N, C), dtype=f32) for _ in range(4)]
            gq = rb
            while gq + rg + 3 * tr < re:
                for k in range(4):
                    st[k] = (st[k] + rows[:, gq + rg + k * tr]).astype(f32)
                gq += 4 * tr
            while gq + rg < re:
                st[0] = (st[0] + rows[:, gq + rg]).astype(f32)
                gq += tr
            a = ((st[0] + st[1]).astype(f32) + (st[2] + st[3]).astype(f32)).astype(f32)
            blk = a if first else (blk + a).astype(f32)
            first = False
        tot += blk.astype(f64)
    return (tot * f64(f32(scale))).astype(f32)


# =================================================================== softmax_rows ============================================
SOFTMAX_C = (1,) + CLASSES
SOFTMAX_FAMILIES = ("trained", "uniform", "saturated", "offset", "ties")
SOFTMAX_M = {1: (1, 1, 1), 713: (1, 23, 31)}        # M -> the make_case shape that gives M rows
SOFTMAX_STRIDE = (GRID_CAP + 5, 2)


def softmax_case(family, C, M):
    """rows [M, C] float32 of loss_bounds.make_case"""
    z, _ = make_case(family, C, SOFTMAX_M[M])
    return np.ascontiguousarray(z.transpose(0, 2, 3, 1).reshape(M, C))


def softmax_ref64(z):
    zd = z.astype(f64)
    e = np.exp(zd - zd.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


def emu_softmax_rows(z):
    """k_softmax_rows: m = fmaxf over the row, s += expf(z_c - m) in order, expf(z_c - m) / s (a correctly rounded expf)"""
    m = z.max(1, keepdims=True)
    e = np.exp((z - m).astype(f32).astype(f64)).astype(f32)
    s = np.zeros(z.shape[0], dtype=f32)
    for c in range(z.shape[1]):
        s = (s + e[:, c]).astype(f32)
    return (e / s[:, None]).astype(f32)


def softmax_excess(got, z):
    """-> (element excess against E_prob(C), row-sum excess against (C + 1) E_prob(C))"""
    C = z.shape[1]
    ref = softmax_ref64(z)
    got = np.asarray(got, dtype=f64)
    if not np.isfinite(got).all():
        return math.inf, math.inf
    return float(np.abs(got - ref).max() / E_prob(C)), float(np.abs(got.sum(1) - 1.0).max() / ((C + 1) * E_prob(C)))


# =================================================================== dense_small ==============================================
DENSE_M = (1, 2, 5, 16)
DENSE_K = (4, 252, 256, 260, 2048)
DENSE_COUT = (1, 3, 4, 6, 256)
DENSE_FAMILIES = ("normal", "pooled")


def dense_case(family, M, K, Cout, seed=0):
    """x [M, K], w [Cout, K], bias [Cout].  pooled: the rows are one vector times (1 + 1 % noise), the pooled rows it serves"""
    rng = np.random.default_rng([seed, 15, DENSE_FAMILIES.index(family), M, K, Cout])
    x = rng.standard_normal((M, K), dtype=f32)
    if family == "pooled":
        x = (np.abs(x[:1]) * (f32(1) + f32(0.01) * rng.standard_normal((M, K), dtype=f32))).astype(f32)
    return x, (rng.standard_normal((Cout, K), dtype=f32) / f32(math.sqrt(K))).astype(f32), rng.standard_normal(Cout, dtype=f32)


def dense_ref64(x, w, bias):
    """-> y64 [M, Cout] and sum |x| |w| (the bias is added exactly in the kernel's double, so it carries no term)"""
    y = x.astype(f64) @ w.astype(f64).T + (0.0 if bias is None else bias.astype(f64))
    return y, np.abs(x).astype(f64) @ np.abs(w).astype(f64).T + (0.0 if bias is None else np.abs(bias).astype(f64))


def emu_dense(x, w, bias):
    return dense_ref64(x, w, bias)[0].astype(f32)


def dense_excess(got, x, w, bias):
    """the documented correctly rounded result: |y - y64| <= EPS |y64| + K 2^-53 sum |x| |w|"""
    y, a = dense_ref64(x, w, bias)
    return rel_excess(got, y, EPS * np.abs(y) + x.shape[1] * 2.0 ** -53 * a + 1e-300)


# =================================================================== optimizers and EMA ======================================
OPT_N = (1, 255, 257, 1000)
OPT_STRIDE_N = GRID_CAP + 3
OPT_STRIDE_SEGS = (GRID_CAP - 2, GRID_CAP + 1)          # b1 and b2 on either side of 2^20


def seg_table(n):
    """(b1, b2) in (0, 0), (n, n), (1, n - 1), (100, 100), (77, 301), kept where 0 <= b1 <= b2 <= n"""
    out = []
    for b in ((0, 0), (n, n), (1, n - 1), (100, 100), (77, 301)):
        if 0 <= b[0] <= b[1] <= n and b not in out:
            out.append(b)
    return out


SGD_SCALES = (1.0, 0.125, 1.0 / 3)
SGD_DECAYS = (0.0, 5e-4)
SGD_STEPS = 3
SGD_LRS = (0.01, 0.1, 0.05)
SGD_MOMENTUM = 0.9
SGD_FAULTS = ("segment_off_by_one",)
ADAM_BETAS = ((0.9, 0.99), (0.9, 0.999))
ADAM_STEPS = 5
ADAM_LRS = (1e-3, 1e-2, 5e-3)
ADAM_EPS = 1e-8
ADAM_FAULTS = ("fp32_one_minus_beta",)
EMA_DECAYS = (0.0, 0.5, 0.99, 0.999, 1.0 - 1.0 / 7)


def opt_case(n, steps, seed=0):
    """p [n] and one gradient per step, float32"""
    rng = np.random.default_rng([seed, 16, n, steps])
    return rng.standard_normal(n, dtype=f32), [rng.standard_normal(n, dtype=f32) for _ in range(steps)]


def seg_lr(n, b1, b2, lrs, fault=None):
    """the per-element learning rate of the arena kernels: i < b1 ? lr0 : (i < b2 ? lr1 : lr2), as float32"""
    i = np.arange(n)
    if fault == "segment_off_by_one":
        return np.where(i <= b1, f32(lrs[0]), np.where(i <= b2, f32(lrs[1]), f32(lrs[2]))).astype(f32)
    return np.where(i < b1, f32(lrs[0]), np.where(i < b2, f32(lrs[1]), f32(lrs[2]))).astype(f32)


def _groups(t, b1, b2, lrs):
    """three torch parameter groups over the segments of a flat tensor (empty segments left out)"""
    ps, groups = [], []
    for lo, hi, lr in ((0, b1, lrs[0]), (b1, b2, lrs[1]), (b2, t.numel(), lrs[2])):
        if hi > lo:
            p = torch.nn.Parameter(t[lo:hi].clone())
            ps.append((lo, hi, p))
            groups.append(dict(params=[p], lr=float(f32(lr))))
    return ps, groups


def sgd_ref64(p, grads, b1, b2, lrs, momentum, wd, gscale):
    """torch.optim.SGD in float64 with three parameter groups, every hyper-parameter the float32 the kernel receives, the
    gradient times grad_scale -> per step (p, buf, unit), unit = |p| + lr (|buf| + |g gscale| + wd |p|) of the step's inputs"""
    n = p.size
    ps, groups = _groups(torch.from_numpy(p).double(), b1, b2, lrs)
    opt = torch.optim.SGD(groups, lr=1.0, momentum=float(f32(momentum)), weight_decay=float(f32(wd)))
    lr = seg_lr(n, b1, b2, lrs).astype(f64)
    out, buf = [], np.zeros(n)
    cur = p.astype(f64)
    for g in grads:
        gs = g.astype(f64) * float(f32(gscale))
        unit = np.abs(cur) + lr * (np.abs(buf) + np.abs(gs) + float(f32(wd)) * np.abs(cur))
        for lo, hi, q in ps:
            q.grad = torch.from_numpy(gs[lo:hi].copy())
        opt.step()
        cur, buf = np.empty(n), np.empty(n)
        for lo, hi, q in ps:
            cur[lo:hi] = q.detach().numpy()
            buf[lo:hi] = opt.state[q]["momentum_buffer"].numpy()
        out.append((cur.copy(), buf.copy(), unit))
    return out


def emu_sgd(p, grads, b1, b2, lrs, momentum, wd, gscale, fault=None):
    """k_sgd: every operation an explicit round-to-nearest fp32 one -> per step (p, buf)"""
    lr = seg_lr(p.size, b1, b2, lrs, fault)
    mom, wd, gs = f32(momentum), f32(wd), f32(gscale)
    out, buf, cur = [], np.zeros_like(p), p.copy()
    for k, g in enumerate(grads):
        gv = ((g * gs).astype(f32) + (wd * cur).astype(f32)).astype(f32)
        buf = gv if k == 0 else ((mom * buf).astype(f32) + gv).astype(f32)
        cur = (cur - (lr * buf).astype(f32)).astype(f32)
        out.append((cur.copy(), buf.copy()))
    return out


def torch_sgd_fp32(p, grads, b1, b2, lrs, momentum, wd, gscale):
    ps, groups = _groups(torch.from_numpy(p.copy()), b1, b2, lrs)
    opt = torch.optim.SGD(groups, lr=1.0, momentum=float(f32(momentum)), weight_decay=float(f32(wd)))
    out = []
    for g in grads:
        gs = (g * f32(gscale)).astype(f32)
        for lo, hi, q in ps:
            q.grad = torch.from_numpy(gs[lo:hi].copy())
        opt.step()
        cur, buf = np.empty(p.size, dtype=f32), np.empty(p.size, dtype=f32)
        for lo, hi, q in ps:
            cur[lo:hi], buf[lo:hi] = q.detach().numpy(), opt.state[q]["momentum_buffer"].numpy()
        out.append((cur, buf))
    return out


SGD_COUNT = 7       # g * gscale, wd * p, their sum, mom * buf, its sum with g, lr * buf, p - that: each at most one unit


def E_sgd():
    return EPS * _b(SGD_COUNT, CAL_SGD)


def sgd_excess(got, ref):
    """got: per step (p, buf) of an implementation, ref: sgd_ref64's list.  The rounding of step s reaches the parameter of every
    later step with a weight of at most 1 (through buf with momentum < 1), so the bound of p after step t is
    E_sgd() sum_{s <= t} (t - s + 1) unit_s; buf is held to the same sum over lr (it is what lr multiplies)"""
    worst = 0.0
    for t in range(len(ref)):
        acc = sum((t - s + 1) * ref[s][2] for s in range(t + 1))
        worst = max(worst, rel_excess(got[t][0], ref[t][0], E_sgd() * acc + 1e-300))
    return worst


def adam_ref64(p, grads, b1, b2, lrs, betas, eps, gscale=1.0):
    """torch.optim.Adam in float64, constructed with the Python-double betas, three parameter groups, weight decay 0 -> per step
    dict(p, m, v)"""
    n = p.size
    ps, groups = _groups(torch.from_numpy(p).double(), b1, b2, lrs)
    opt = torch.optim.Adam(groups, lr=1.0, betas=(float(betas[0]), float(betas[1])), eps=float(f32(eps)))
    out = []
    for g in grads:
        gs = g.astype(f64) * float(f32(gscale))
        for lo, hi, q in ps:
            q.grad = torch.from_numpy(gs[lo:hi].copy())
        opt.step()
        st = dict(p=np.empty(n), m=np.empty(n), v=np.empty(n))
        for lo, hi, q in ps:
            st["p"][lo:hi] = q.detach().numpy()
            st["m"][lo:hi] = opt.state[q]["exp_avg"].numpy()
            st["v"][lo:hi] = opt.state[q]["exp_avg_sq"].numpy()
        out.append(st)
    return out


def adam_host_args(betas, step):
    """what ParamArena.adam_step hands to u2pl_adam_step_f32 as Python floats (ctypes rounds each ONCE to float32):
    beta1, 1 - beta1, beta2, 1 - beta2, bias_correction1, bias_correction2_sqrt"""
    b1, b2 = float(betas[0]), float(betas[1])
    return b1, 1.0 - b1, b2, 1.0 - b2, 1.0 - b1 ** step, math.sqrt(1.0 - b2 ** step)


def emu_adam(p, grads, b1, b2, lrs, betas, eps, gscale=1.0, wd=0.0, fault=None):
    """k_adam in fp32, operation by operation (IEEE division and square root).  fp32_one_minus_beta: the kernel before the fix,
    which formed 1.0f - beta on the device"""
    lr = seg_lr(p.size, b1, b2, lrs)
    cur, m, v = p.copy(), np.zeros_like(p), np.zeros_like(p)
    eps, gs, wd = f32(eps), f32(gscale), f32(wd)
    out = []
    for k, g in enumerate(grads):
        be1, om1, be2, om2, bc1, bc2s = (f32(a) for a in adam_host_args(betas, k + 1))
        if fault == "fp32_one_minus_beta":
            om1, om2 = f32(f32(1) - be1), f32(f32(1) - be2)
        gv = ((g * gs).astype(f32) + (wd * cur).astype(f32)).astype(f32)
        m = (m + (om1 * (gv - m).astype(f32)).astype(f32)).astype(f32)
        v = ((v * be2).astype(f32) + (om2 * (gv * gv).astype(f32)).astype(f32)).astype(f32)
        denom = ((np.sqrt(v).astype(f32) / bc2s).astype(f32) + eps).astype(f32)
        cur = (cur - ((lr / bc1).astype(f32) * (m / denom).astype(f32)).astype(f32)).astype(f32)
        out.append(dict(p=cur.copy(), m=m.copy(), v=v.copy()))
    return out


def torch_adam_fp32(p, grads, b1, b2, lrs, betas, eps, gscale=1.0):
    ps, groups = _groups(torch.from_numpy(p.copy()), b1, b2, lrs)
    opt = torch.optim.Adam(groups, lr=1.0, betas=(float(betas[0]), float(betas[1])), eps=float(f32(eps)))
    out = []
    for g in grads:
        gs = (g * f32(gscale)).astype(f32)
        for lo, hi, q in ps:
            q.grad = torch.from_numpy(gs[lo:hi].copy())
        opt.step()
        st = dict(p=np.empty(p.size, dtype=f32), m=np.empty(p.size, dtype=f32), v=np.empty(p.size, dtype=f32))
        for lo, hi, q in ps:
            st["p"][lo:hi] = q.detach().numpy()
            st["m"][lo:hi] = opt.state[q]["exp_avg"].numpy()
            st["v"][lo:hi] = opt.state[q]["exp_avg_sq"].numpy()
        out.append(st)
    return out


def adam_v_count(t):
    """exp_avg_sq after step t relative to itself (every term is positive): the new term carries g * gscale twice (2), the
    square (1), the product with 1 - beta2 (1) and that weight's own rounding (1); the old value its earlier error, the
    product with beta2 (1) and the rounding of beta2 to float32 (1; the reference holds the double); the sum one more:
    c_1 = 6, c_t = max(5, c_{t-1} + 2) + 1 = c_{t-1} + 3"""
    return 6 + 3 * (t - 1)


def adam_m_count(t, beta1):
    """exp_avg after step t relative to G = max_s |g_s|: per step, scaled by w = 1 - beta1: g * gscale (1), g - m (2: its size is
    at most 2 G), the product (2) and the weight's rounding (2), plus the final add (1 on |m| <= G); earlier errors shrink by
    beta1: at most t (1 + 7 w)"""
    return t * (1 + 7 * (1 - beta1))


def adam_u_count(t, betas):
    """the update u = (lr / bc1) m / (sqrt(v) / bc2s + eps) relative to lr.  |m| / bc1 <= G and sqrt(v) / bc2s >= G / kappa with
    kappa = sqrt(bc2 / (1 - beta2)), so |u| <= kappa lr; m's error (adam_m_count G) enters divided by bc1 and by the
    denominator: kappa adam_m_count / bc1; the relative errors of v (half of adam_v_count through the root), the root, the two
    divisions, the sum with eps, lr / bc1 and the product (6) scale with |u| <= kappa lr"""
    bc1, bc2 = 1 - betas[0] ** t, 1 - betas[1] ** t
    kappa = math.sqrt(bc2 / (1 - betas[1]))
    return kappa * (adam_m_count(t, betas[0]) / bc1 + 0.5 * adam_v_count(t) + 6)


def adam_measure(got, ref, p0, grads, lr):
    """-> dict(exp_avg_sq, exp_avg, update): the largest error over the steps in the units of the CAL_ADAM_* constants.  update:
    |(p_t - p_{t-1}) - the float64 one| beyond the rounding EPS |p_t| of the stored parameter, in units of EPS lr (FINDING 2)"""
    out = dict(exp_avg_sq=0.0, exp_avg=0.0, update=0.0)
    G = np.zeros(p0.size)
    prev_g, prev_r = p0.astype(f64), p0.astype(f64)
    for t, (a, r) in enumerate(zip(got, ref)):
        G = np.maximum(G, np.abs(grads[t].astype(f64)))
        out["exp_avg_sq"] = max(out["exp_avg_sq"], rel_excess(a["v"], r["v"], EPS * r["v"]))
        out["exp_avg"] = max(out["exp_avg"], rel_excess(a["m"], r["m"], EPS * G + 1e-300))
        du, du64 = a["p"].astype(f64) - prev_g, r["p"] - prev_r
        over = np.maximum(np.abs(du - du64) - EPS * np.abs(r["p"]), 0.0)
        out["update"] = max(out["update"], float((over / (EPS * lr)).max()))
        prev_g, prev_r = a["p"].astype(f64), r["p"]
    return out


def adam_excess(got, ref, p0, grads, lr, betas):
    """-> dict(exp_avg_sq, exp_avg, update) of excesses (> 1: out of bound), each step against its own count"""
    out = dict(exp_avg_sq=0.0, exp_avg=0.0, update=0.0)
    G = np.zeros(p0.size)
    prev_g, prev_r = p0.astype(f64), p0.astype(f64)
    for t, (a, r) in enumerate(zip(got, ref)):
        G = np.maximum(G, np.abs(grads[t].astype(f64)))
        out["exp_avg_sq"] = max(out["exp_avg_sq"], rel_excess(a["v"], r["v"], EPS * _b(adam_v_count(t + 1), CAL_ADAM_V) * r["v"]))
        out["exp_avg"] = max(out["exp_avg"],
                             rel_excess(a["m"], r["m"], EPS * _b(adam_m_count(t + 1, betas[0]), CAL_ADAM_M) * G + 1e-300))
        du, du64 = a["p"].astype(f64) - prev_g, r["p"] - prev_r
        bound = EPS * (np.abs(r["p"]) + _b(adam_u_count(t + 1, betas), CAL_ADAM_U) * lr)
        out["update"] = max(out["update"], rel_excess(du, du64, bound))
        prev_g, prev_r = a["p"].astype(f64), r["p"]
    return out


def ema_args(decay):
    """what ParamArena.ema_from hands over: float(decay), float(1 - decay), each rounded once to float32"""
    return f32(float(decay)), f32(1.0 - float(decay))


def ema_ref64(t, s, decay):
    d, omd = (f64(a) for a in ema_args(decay))
    return d * t.astype(f64) + omd * s.astype(f64), np.abs(d * t.astype(f64)) + np.abs(omd * s.astype(f64))


def emu_ema(t, s, decay):
    d, omd = ema_args(decay)
    return ((d * t).astype(f32) + (omd * s).astype(f32)).astype(f32)


EMA_COUNT = 3       # two products and a sum, on |d t| + |(1 - d) s|


def E_ema():
    return EPS * _b(EMA_COUNT, CAL_EMA)


# =================================================================== cutmix / cutout / classmix / label presence ===============
MIX_B = (1, 2, 3)
MIX_C = (1, 3)
MIX_HW = ((1, 1), (5, 7), (33, 35))
MIX_LABELS = (0, 1, 5, 18, 63, 64, 100, 254, 255)       # 255 = ignore; 63: the last selectable class; >= 64 never selected
MIX_STRIDE = (2, 1, 725, 724)                           # B H W = 2^20 + 1224: just past the cap
MIX_FAULTS = ("box_includes_end_row", "label_cast_int8_before_blend")
PRESENCE_HW = (1, 255, 257, 256 * 256 + 5)
PRESENCE_LABELS = (0, 63, 64, 255)


def mix_boxes(B, H, W):
    """per image, cycling: empty (y0 == y1), the whole image, one pixel in the top-left corner, one touching the bottom-right
    edge -> list of B-lists of (y0, y1, x0, x1)"""
    kinds = [(H // 2, H // 2, 0, W), (0, H, 0, W), (0, 1, 0, 1), (H - max(1, H // 3), H, W - max(1, W // 2), W)]
    return [[kinds[(k + i) % 4] for i in range(B)] for k in range(4)]


def mix_case(B, C, H, W, seed=0):
    rng = np.random.default_rng([seed, 17, B, C, H, W])
    img = rng.standard_normal((B, C, H, W), dtype=f32)
    lab = np.asarray(MIX_LABELS, dtype=np.int64)[rng.integers(0, len(MIX_LABELS), (B, H, W))]
    lab.reshape(-1)[:len(MIX_LABELS)] = MIX_LABELS[:lab.size]          # every label value where the image has room
    conf = rng.random((B, H, W), dtype=f32)
    return img, lab, conf


def mix_selections(B):
    """selection words with bit 0, bit 63 and some between, one per image"""
    words = [np.uint64(1), np.uint64(1) << np.uint64(63), (np.uint64(1) << np.uint64(5)) | (np.uint64(1) << np.uint64(18)),
             np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64(0)]
    return [np.array([words[(k + i) % len(words)] for i in range(B)], dtype=np.uint64) for k in range(len(words))]


def _box_mask(B, H, W, boxes, fault=None):
    m = np.zeros((B, H, W), dtype=f32)
    for i, (y0, y1, x0, x1) in enumerate(boxes):
        m[i, y0:min(H, y1 + 1) if fault == "box_includes_end_row" else y1, x0:x1] = 1
    return m


def mix_ref(mode, img, lab, conf, boxes=None, sel=None, fault=None):
    """the reference expression a * m + b * (1 - m) in fp32 (generate_unsup_data).  cutmix: m = 0 inside box_i, b = sample i + 1;
    cutout: b = 0 and the label 255 inside the box; classmix: m = [label_i selected], the labels through float and back"""
    B, C, H, W = img.shape
    nxt = (np.arange(B) + 1) % B
    one = f32(1)
    if mode == "cutmix":
        m = one - _box_mask(B, H, W, boxes, fault)
        return ((img * m[:, None] + img[nxt] * (one - m)[:, None]).astype(f32), np.where(m > 0, lab, lab[nxt]),
                (conf * m + conf[nxt] * (one - m)).astype(f32))
    if mode == "cutout":
        m = one - _box_mask(B, H, W, boxes, fault)
        return (img * m[:, None]).astype(f32), np.where(m > 0, lab, 255), (conf * m).astype(f32)
    inside = (lab >= 0) & (lab < 64)
    bit = (sel[:, None, None] >> np.where(inside, lab, 0).astype(np.uint64)) & np.uint64(1)
    m = (inside & (bit == 1)).astype(f32)
    la, lb = lab, lab[nxt]
    if fault == "label_cast_int8_before_blend":
        la, lb = la.astype(np.int8), lb.astype(np.int8)
    ol = (la.astype(f32) * m + lb.astype(f32) * (one - m)).astype(np.int64)
    return (img * m[:, None] + img[nxt] * (one - m)[:, None]).astype(f32), ol, (conf * m + conf[nxt] * (one - m)).astype(f32)


def presence_case(B, HW, seed=0):
    """labels of PRESENCE_LABELS, image i without PRESENCE_LABELS[i % 4]; a single pixel holds PRESENCE_LABELS[i % 4] itself"""
    rng = np.random.default_rng([seed, 18, B, HW])
    lab = np.empty((B, HW), dtype=np.int64)
    for i in range(B):
        pool = [v for k, v in enumerate(PRESENCE_LABELS) if k != i % 4] if HW > 1 else [PRESENCE_LABELS[i % 4]]
        lab[i] = np.asarray(pool, dtype=np.int64)[rng.integers(0, len(pool), HW)]
        if HW >= 255:
            lab[i, HW - 1] = pool[0]            # the last pixel (the tail of the last block) holds a class of its own ...
            lab[i, :HW - 1][lab[i, :HW - 1] == pool[0]] = pool[1]      # ... that no other pixel has
    return lab


def presence_ref(lab):
    out = np.zeros(lab.shape[0], dtype=np.uint64)
    for i in range(lab.shape[0]):
        for v in np.unique(lab[i]):
            if 0 <= v < 64:
                out[i] |= np.uint64(1) << np.uint64(v)
    return out


# =================================================================== sliding-window accumulate / normalize ====================
WIN_C = (1, 19)
WIN_ACC = (9, 11)
# (h0, w0, hc, wc), in call order: one overlapping another, one in each corner, one covering everything
WINDOWS = ((2, 3, 4, 5), (4, 5, 4, 5), (0, 0, 3, 4), (0, 7, 3, 4), (6, 0, 3, 4), (6, 7, 3, 4), (0, 0, 9, 11))


def window_case(C, seed=0):
    rng = np.random.default_rng([seed, 19, C])
    return [rng.standard_normal((C, w[2], w[3]), dtype=f32) for w in WINDOWS]


def emu_windows(C, srcs, windows=WINDOWS, acc=WIN_ACC):
    """the sequential fp32 adds in call order -> pred [C, H, W], count [H, W]"""
    pred, count = np.zeros((C,) + tuple(acc), dtype=f32), np.zeros(acc, dtype=f32)
    for (h0, w0, hc, wc), s in zip(windows, srcs):
        pred[:, h0:h0 + hc, w0:w0 + wc] = (pred[:, h0:h0 + hc, w0:w0 + wc] + s).astype(f32)
        count[h0:h0 + hc, w0:w0 + wc] += f32(1)
    return pred, count


# =================================================================== calibration: what torch's fp32 reaches =====================
def _ratio(got, ref, unit):
    return rel_excess(got, ref, EPS * np.asarray(unit, dtype=f64) + 1e-300)


def measure_pool_bwd(form="torch"):
    worst = 0.0
    for shape in POOL_SHAPES:
        for fam in POOL_FAMILIES:
            x, g = pool_case(fam, shape)
            _, tap, dx, unit = pool_ref64(x, g)
            got = torch_pool_bwd_fp32(x, g) if form == "torch" else emu_pool_bwd(g, emu_pool_fwd(x)[1], shape[2], shape[3])
            worst = max(worst, _ratio(got, dx, unit))
    return worst


def measure_bilr(form="torch", C=4, N=1):
    fwd = bwd = 0.0
    for lo, hi in BILR_SHAPES:
        x, _ = bilr_case(lo, hi, N, C)
        got = torch_bilr_fwd_fp32(x, *hi) if form == "torch" else emu_bilr_fwd(x, *hi)
        fwd = max(fwd, _ratio(got, bilinear_fwd64(x, *hi), bilr_fwd_unit(x, *hi)))
        if form == "torch":
            bwd = max(bwd, measure_bilinear(lo, hi, "torch"))
        else:
            _, g = bilr_case(lo, hi, N, C)
            ref, unit = bilinear_bwd64(g, *lo)
            bwd = max(bwd, _ratio(emu_bilr_bwd(g, *lo), ref, unit))
    return fwd, bwd


def measure_gap(form="torch"):
    """-> (forward in EPS mean |x|, backward in EPS |g| / HW, column sums in EPS sum |g|)"""
    fwd = bwd = col = 0.0
    for shape in GAP_SHAPES:
        x, g = gap_case(shape)
        HW = shape[2] * shape[3]
        x64 = x.astype(f64)
        if form == "torch":
            xt = torch.from_numpy(x).requires_grad_(True)
            y = F.adaptive_avg_pool2d(xt, 1)
            y.backward(torch.from_numpy(g)[:, :, None, None])
            got_f, got_b = y.detach().numpy()[:, :, 0, 0], xt.grad.numpy()
            got_c = torch.from_numpy(x).sum((2, 3)).numpy()
        else:
            got_f, got_c = emu_colsum(x, 1.0 / HW), emu_colsum(x, 1.0)
            got_b = np.broadcast_to(emu_broadcast(g, 1.0 / HW, 1, g.shape[0])[:, :, None, None], shape)
        fwd = max(fwd, _ratio(got_f, x64.mean((2, 3)), np.abs(x64).mean((2, 3))))
        col = max(col, _ratio(got_c, x64.sum((2, 3)), np.abs(x64).sum((2, 3))))
        bwd = max(bwd, _ratio(got_b, np.broadcast_to((g.astype(f64) / HW)[:, :, None, None], shape),
                              np.broadcast_to((np.abs(g.astype(f64)) / HW)[:, :, None, None], shape)))
    return fwd, bwd, col


def measure_sgd(form="torch", ns=(257, 1000)):
    worst = 0.0
    for n in ns:
        p, grads = opt_case(n, SGD_STEPS)
        for b1, b2 in seg_table(n):
            for gs in SGD_SCALES:
                for wd in SGD_DECAYS:
                    a = (p, grads, b1, b2, SGD_LRS, SGD_MOMENTUM, wd, gs)
                    ref = sgd_ref64(*a)
                    got = torch_sgd_fp32(*a) if form == "torch" else emu_sgd(*a)
                    for t in range(SGD_STEPS):
                        acc = sum((t - s + 1) * ref[s][2] for s in range(t + 1))
                        worst = max(worst, _ratio(got[t][0], ref[t][0], acc))
    return worst


def measure_adam(betas, form="torch", n=1000, fault=None):
    p, grads = opt_case(n, ADAM_STEPS)
    b1, b2 = 77, 301
    ref = adam_ref64(p, grads, b1, b2, ADAM_LRS, betas, ADAM_EPS)
    a = (p, grads, b1, b2, ADAM_LRS, betas, ADAM_EPS)
    got = torch_adam_fp32(*a) if form == "torch" else emu_adam(*a, fault=fault)
    return adam_measure(got, ref, p, grads, seg_lr(n, b1, b2, ADAM_LRS).astype(f64))


def measure_ema(form="torch", n=1000):
    worst = 0.0
    t, (s,) = opt_case(n, 1, seed=3)
    for d in EMA_DECAYS:
        ref, unit = ema_ref64(t, s, d)
        if form == "torch":
            da, oa = ema_args(d)
            got = (torch.from_numpy(t) * float(da) + torch.from_numpy(s) * float(oa)).numpy()
        else:
            got = emu_ema(t, s, d)
        worst = max(worst, _ratio(got, ref, unit))
    return worst
