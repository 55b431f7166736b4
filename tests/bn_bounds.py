"""Element-wise float64 error bounds of the train- and eval-mode BatchNorm arithmetic, shared by the
CPU restatement (tests/test_bn_bounds_cpu.py) and the GPU route tests (tests/test_gpu_bn_bounds.py).  Not a conftest: imported by
name.

Reference (per channel, the kernel's fp32 inputs promoted to float64): mu = mean x, v = two-pass biased variance,
iota = 1 / sqrt(v + eps), y = gamma (x - mu) iota + beta (+ res, ReLU, x drop[n, c]); backward g = dy mask drop, S0 = sum g,
S1 = sum g xhat, dx = gamma iota (g - S0/M - xhat S1/M), dgamma = S1, dbeta = S0, dres = g; running_mean' = (1-m) rm + m mu,
running_var' = (1-m) rv + m v M/(M-1); eval mode iota = 1 / sqrt(running_var + eps), dx = gamma iota g.

Bound (first order in EPS = 2^-24; the float64 parts in units of D64 = 2^-53).  The statistics are fp32 sums of d = x - p and d^2
(p: the pivot, the running_mean the kernel read) finished in double as var = m2 - m1^2, m1 = S1/M, m2 = S2/M.  If every term of a
sum passes through at most L fp32 roundings (its own x - p, the additions of the route's partial sums, and one unit for the double
finish: (nblk + 16) 2^-53 < 2^-24), then

    |m1^ - m1| <= e1 = L EPS mean|d|                 |m2^ - m2| <= e2 = (L + 2) EPS mean d^2     (d^2: 2 more roundings)
    |mu^ - mu| <= e1 + EPS |mu|                      |v^ - v|   <= e2 + e1 (2 |m1| + e1)

|m1| mean|d| <= mean d^2, so the variance error is of the order 3 L EPS mean (x - p)^2 = 3 L EPS (1 + R^2) sigma^2 with
R = |mu - p| / sigma: the pivot term is kept explicit, never folded into a constant.  Epilogues that shift by a bias first
(v = fl(acc + fl(b - p)) against the stored y = fl(acc + b)) add an absolute error a_i = EPS (|b - p| + |x_i|) to each term.
iota's error is the exact interval of 1/sqrt over [v - e_v, v + e_v] (no first-order step: at R = 1000 e_v exceeds v), widened by
the one rounding of the cast.  The outputs carry those errors plus the fp32 roundings of each kernel's own expression, counted
from the code (k_bn_apply: 4 roundings, + 1 for res, + 1 for drop; k_bn_bwd_apply: see bwd_ref_bound).  ReLU is 1-Lipschitz; the
drop scale multiplies the bound.  Where |pre-activation| <= its bound the kernel's ReLU mask may differ from the float64 one;
everywhere else the two masks must be identical.

The L of each statistics route is derived from the code next to its definition below."""
import numpy as np
import torch

from split_bounds import EPS, excess, recorded_calls  # noqa: F401  (re-exported: one definition for both bound modules)

D64 = 2.0 ** -53
SMALL_M = 64          # u2pl_bn_stats_f32: M <= 64 rows take the float64 two-pass kernel (csrc/nn.hip: k_bn_stats_small)


# ---- L: the longest fp32 rounding chain of one term, per statistics route -----------------------------------------------------
def colreduce_geometry(M, C):
    """k_colreduce_partial's launch (csrc/nn.hip: colreduce_blocks, run_colreduce): nblk row blocks of `per` rows, and per column
    slab of 64 float4 columns the number of row groups tr = 256 / (float4 columns of the slab)"""
    nblk = max(1, min(512, -(-M // 64)))
    per = -(-M // nblk)
    C4 = C // 4
    trs = [256 // min(64, C4 - s) for s in range(0, C4, 64)]
    return nblk, per, trs


def L_colreduce_chain(M, C):
    """roundings of a term after it is formed, in k_colreduce_partial + k_colreduce_final.  A thread owns J = ceil(per / tr) rows
    of its block, spread over four streams (main loop: ceil(J/4) rows each; the tail adds up to 3 more to stream a), then
    (a + b) + (c + d) (2), then row group 0 adds the other tr - 1 groups in order (tr - 1), then the ordered double finish (1)."""
    nblk, per, trs = colreduce_geometry(M, C)
    return max(-(-(-(-per // tr)) // 4) + 3 + 2 + (tr - 1) + 1 for tr in trs)


def L_standalone(M, C):
    """u2pl_bn_stats_f32, M > 64: the term x - p is one rounding in front of the column-reduce chain"""
    return 1 + L_colreduce_chain(M, C)


# igemm_ws.hip (fused statistics behind the stores): fl(acc + sh) (1), 16 register values in order (15), the two lane halves (1),
# the four 32-row blocks of the 128-row tile in order (3), the double finish (1)
L_IGEMM_WS = 1 + 15 + 1 + 3 + 1
# conv.hip (k_conv_igemm statistics; every plan has TM = 2, WM = 2 -- Cout <= 64 -- or TM = 1, WM = 4): fl(acc + sh) (1), TM x 16
# register values in order (<= 31), the lane halves (1), the WM wave blocks in order (<= 3), the double finish (1)
L_CONV = 1 + 31 + 1 + 3 + 1


def wino_tpb(C):
    """tiles per block of the Winograd output transform with statistics (wino.hip: u2pl_wino_stat_blocks)"""
    return max(1, 256 // (C // 4))


def L_wino(mt, C):
    """wino.hip output transform with statistics: fl(y - p) (1), a thread's mt x mt outputs in order (mt^2 - 1), the block's tpb
    tiles in tile order (tpb - 1), the double finish (1)"""
    return 1 + (mt * mt - 1) + (wino_tpb(C) - 1) + 1


# ---- reference and bounds (torch float64, any device) -------------------------------------------------------------------------
def stats_ref(x):
    """x [M, C] float64 -> (mu, two-pass biased variance)"""
    mu = x.mean(0)
    return mu, ((x - mu) ** 2).mean(0)


def stats_bound(x, p, L, shift_err=None):
    """(bound of |mu^ - mu| for the fp32 mean, bound of |v^ - v|, bound of the double mean before its cast) for a route of chain
    length L (None: the float64 two-pass kernel of M <= 64 rows).  x [M, C] float64, p [C] float64: the pivot the kernel read;
    shift_err [M, C]: the a_i of a bias shift."""
    M = x.shape[0]
    mu, _ = stats_ref(x)
    d = x - p
    m1 = mu - p
    d2 = (d * d).mean(0)
    if L is None:
        # k_bn_stats_small: s = sum x, mean = s / M, q = sum (x - mean)^2 in float64, then M dm and q + M dm^2 (dm = mean - p)
        # through the same double finalisation: <= (M + 4) roundings of mean|x| + |p| in m1, (M + 16) of mean d^2 in m2 - m1^2
        e1 = (M + 4) * D64 * (x.abs().mean(0) + p.abs())
        e_var = (M + 16) * D64 * d2 + e1 * (4 * m1.abs() + e1)
    else:
        e1 = L * EPS * d.abs().mean(0)
        e2 = (L + 2) * EPS * d2
        if shift_err is not None:
            e1 = e1 + shift_err.mean(0)
            e2 = e2 + 2 * (d.abs() * shift_err).mean(0) + (shift_err * shift_err).mean(0)
        e_var = e2 + e1 * (2 * m1.abs() + e1)
    e1 = e1 + D64 * (mu.abs() + p.abs())          # mu = p + m1 in double
    return e1 + EPS * mu.abs(), e_var, e1


def bias_shift_err(x, bias, p):
    """a_i of the epilogues that shift by fl(b - p) before adding the accumulator (igemm_ws.hip, conv.hip)"""
    return EPS * ((bias - p).abs() + x.abs())


def invstd_interval(var, e_var, eps):
    """iota = 1/sqrt(var + eps), the largest |iota^ - iota| over [var - e_var, var + e_var] and the cast, and iota^'s upper end"""
    iota = 1.0 / torch.sqrt(var + eps)
    hi = 1.0 / torch.sqrt((var - e_var).clamp_min(0.0) + eps) * (1 + EPS + 4 * D64)
    lo = 1.0 / torch.sqrt(var + e_var + eps) * (1 - EPS - 4 * D64)
    return iota, torch.maximum(hi - iota, iota - lo), hi


def apply_ref_bound(x, mu, iota, e_mu, e_iota, iota_hi, gamma, beta, res=None):
    """pre-activation y = gamma (x - mu) iota + beta (+ res) and its bound.  k_bn_apply rounds x - mu, * invstd, * gamma, + beta
    (each at most EPS of a term <= A = |gamma| (|x - mu| + e_mu) iota_hi, the last of A + |beta|), and + res once more"""
    xc = x - mu
    pre = gamma * xc * iota + beta
    A = gamma.abs() * (xc.abs() + e_mu) * iota_hi
    b = gamma.abs() * (e_mu * iota_hi + xc.abs() * e_iota) + EPS * (4 * A + beta.abs())
    if res is not None:
        pre = pre + res
        b = b + EPS * (A + beta.abs() + res.abs())
    return pre, b


def finish_y(pre, b, relu, drop_rows):
    """ReLU (1-Lipschitz: the bound stays) and the drop scale (multiplies the bound, + one rounding of the product)"""
    y = pre.clamp_min(0.0) if relu else pre
    if drop_rows is not None:
        y = y * drop_rows
        b = b * drop_rows.abs() + EPS * (y.abs() + b * drop_rows.abs())
    return y, b


def mask_mismatch(pre, b_pre, y_kernel, drop_rows=None):
    """elements where the kernel's ReLU decision differs from the float64 one although |pre| exceeds its bound"""
    decided = pre.abs() > b_pre
    if drop_rows is not None:
        decided = decided & (drop_rows != 0)
    return int((decided & ((y_kernel > 0) != (pre > 0))).sum())


def running_ref_bound(rm0, rv0, mu, var, M, momentum, e_m1, e_var):
    """running_mean' / running_var' of k_bn_finalize (double, then one rounding to fp32) and their bounds; momentum is the fp32
    the kernel reads"""
    m = float(np.float32(momentum))
    rm = (1 - m) * rm0 + m * mu
    rv = (1 - m) * rv0 + m * var * M / (M - 1)
    brm = m * e_m1 + EPS * rm.abs() + 4 * D64 * (rm0.abs() + mu.abs())
    brv = m * M / (M - 1) * e_var + EPS * rv.abs() + 4 * D64 * (rv0.abs() + 2 * var)
    return rm, brm, rv, brv


def bwd_ref_bound(x, dy, mask, drop_rows, mu, iota, e_mu, e_iota, iota_hi, gamma, Lc):
    """train-mode backward: dict name -> (ref, bound) for dx, dres, S0 (dbeta), S1 (dgamma).  Lc: L_colreduce_chain of the
    backward sums.  Kernel roundings: g = fl(dy drop) (1, only with drop); xhat = fl(fl(x - mu) invstd) (2); g xhat (1);
    m0 = fl(S0/M), m1 = fl(S1/M) (1 each); dx = fl(fl(gamma invstd) fl(fl(g - m0) - fl(xhat m1))) (4)."""
    M = x.shape[0]
    g = dy * mask
    if drop_rows is not None:
        g = g * drop_rows
    xc = x - mu
    xh = xc * iota
    S0, S1 = g.sum(0), (g * xh).sum(0)
    m0, m1 = S0 / M, S1 / M
    inner = g - m0 - xh * m1
    ag = g.abs()
    e_g = EPS * ag if drop_rows is not None else torch.zeros_like(ag)
    e_xh = e_mu * iota_hi + xc.abs() * e_iota + 2 * EPS * (xc.abs() + e_mu) * iota_hi
    axh = xh.abs() + e_xh
    e_S0 = Lc * EPS * ag.sum(0) + e_g.sum(0)
    e_S1 = (ag * e_xh).sum(0) + (Lc + 1) * EPS * (ag * axh).sum(0) + (e_g * axh).sum(0)
    e_m0, e_m1 = e_S0 / M + EPS * m0.abs(), e_S1 / M + EPS * m1.abs()
    am0, am1 = m0.abs() + e_m0, m1.abs() + e_m1
    e_t = e_xh * am1 + xh.abs() * e_m1 + EPS * axh * am1
    absI = ag + e_g + am0 + axh * am1
    e_in = e_g + e_m0 + e_t + 2 * EPS * absI
    e_dx = gamma.abs() * (iota_hi * e_in + (e_iota + 2 * EPS * iota_hi) * absI)
    return dict(dx=(gamma * iota * inner, e_dx), dres=(g, e_g), S0=(S0, e_S0), S1=(S1, e_S1))


def eval_bwd_ref_bound(dy, mask, drop_rows, iota, e_iota, iota_hi, gamma):
    """eval mode: dx = fl(fl(gamma invstd) g)"""
    g = dy * mask
    if drop_rows is not None:
        g = g * drop_rows
    e_g = EPS * g.abs() if drop_rows is not None else torch.zeros_like(g)
    return gamma * iota * g, gamma.abs() * (g.abs() * (e_iota + 2 * EPS * iota_hi) + iota_hi * e_g)


# ---- the routes' summation orders, emulated in fp32 (numpy) -------------------------------------------------------------------
def _f(a):
    return np.asarray(a, dtype=np.float32)


def emu_colreduce(V):
    """k_colreduce_partial (fp32, the kernel's order) + k_colreduce_final (double): V [M, C] float32 terms -> double [C]"""
    M, C = V.shape
    nblk, per, _ = colreduce_geometry(M, C)
    out = np.zeros(C, dtype=np.float64)
    C4 = C // 4
    for s in range(0, C4, 64):
        cols = slice(4 * s, 4 * min(C4, s + 64))
        tr = 256 // min(64, C4 - s)
        J = -(-per // tr)
        # row b * per + j * tr + rg of block b, thread rg (rows past the block or the matrix: zero, an exact no-op in fp32)
        jr = np.arange(J)[None, :, None] * tr + np.arange(tr)[None, None, :]
        idx = np.arange(nblk)[:, None, None] * per + jr
        ok = (jr < per) & (idx < M)
        T = np.where(ok[..., None], V[np.minimum(idx, M - 1), cols], np.float32(0))      # [nblk][J][tr][c]
        n4 = ok.sum(1) // 4                                                                # main-loop trips per thread
        acc = np.zeros((4,) + T[:, 0].shape, dtype=np.float32)
        for j in range(J):
            stream = np.where(j < 4 * n4, j % 4, 0)[..., None]
            for k in range(4):
                acc[k] = np.where(stream == k, acc[k] + T[:, j], acc[k])
        a = (acc[0] + acc[1]) + (acc[2] + acc[3])
        tot = a[:, 0].copy()
        for k in range(1, tr):
            tot = tot + a[:, k]
        out[cols] = tot.astype(np.float64).sum(0)
    return out


def _conv_tile(T, TM=2, WM=2):
    """conv.hip (k_conv_igemm statistics): per wave block wm, lane half lh sums TM x 16 register values in (a, e) order, rows
    wm 32 TM + a 32 + 4 lh + (e & 3) + 8 (e >> 2); the halves added; the WM blocks added in order.  igemm_ws.hip: TM = 1, WM = 4."""
    blocks = []
    for wm in range(WM):
        halves = []
        for lh in range(2):
            s = np.zeros(T.shape[1], dtype=np.float32)
            for a in range(TM):
                for e in range(16):
                    s = s + T[wm * 32 * TM + a * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh]
            halves.append(s)
        blocks.append(halves[0] + halves[1])
    a = blocks[0]
    for q in range(1, WM):
        a = a + blocks[q]
    return a


def _wino_block(mt, tpb):
    def order(T):      # tpb tiles of mt x mt outputs: each tile summed in output order, the tiles in tile order
        a = np.zeros(T.shape[1], dtype=np.float32)
        for t in range(tpb):
            s = np.zeros(T.shape[1], dtype=np.float32)
            for i in range(mt * mt):
                s = s + T[t * mt * mt + i]
            a = a + s
        return a
    return order


def emulate_stats(route, x, p, acc=None, bias=None, mt=4, drop_last=False):
    """double (S1, S2) of a route for the stored fp32 BatchNorm input x and pivot p (float32).  igemm_ws / conv with a bias:
    acc is the accumulator (x = fl(acc + bias)) and the terms are fl(acc + fl(bias - p)).  drop_last: the mutant that loses the
    last partial block."""
    x, p = _f(x), _f(p)
    if route in ("igemm_ws", "conv") and bias is not None:
        V = _f(_f(acc) + _f(_f(bias) - p))
    else:
        V = _f(x - p)
    V2 = _f(V * V)
    if route == "standalone":
        if drop_last:
            nblk, per, _ = colreduce_geometry(*x.shape)
            V, V2 = V.copy(), V2.copy()
            V[(nblk - 1) * per:] = 0
            V2[(nblk - 1) * per:] = 0
        return emu_colreduce(V), emu_colreduce(V2)
    if route == "igemm_ws":
        order, rows = (lambda T: _conv_tile(T, TM=1, WM=4)), 128
    elif route == "conv":
        order, rows = _conv_tile, 128
    elif route == "wino":
        order, rows = _wino_block(mt, wino_tpb(x.shape[1])), mt * mt * wino_tpb(x.shape[1])
    else:
        raise ValueError(route)
    M, C = V.shape
    nt = -(-M // rows)
    out = []
    for W in (V, V2):
        P = np.zeros((nt * rows, C), dtype=np.float32)
        P[:M] = W
        parts = np.stack([order(P[t * rows:(t + 1) * rows]) for t in range(nt - 1 if drop_last else nt)])
        out.append(parts.astype(np.float64).sum(0))
    return out[0], out[1]


def emulate_small(x, p):
    """k_bn_stats_small: float64 two passes, re-expressed as the shifted sums"""
    x = _f(x).astype(np.float64)
    M = x.shape[0]
    mean = x.sum(0) / M
    q = ((x - mean) ** 2).sum(0)
    dm = mean - _f(p).astype(np.float64)
    return M * dm, q + M * dm * dm


def emulate_finalize(S1, S2, M, p, eps, momentum, rm, rv, fp32=False, count=None, pivot_after=False, swap_m=False,
                     biased_rv=False, eps_outside=False):
    """k_bn_finalize (double) -> fp32 mean, invstd, running_mean', running_var'; the keyword arguments make the mutants"""
    cnt = float(M if count is None else count)
    m = float(np.float32(momentum))
    eps = float(np.float32(eps))
    p = _f(p).astype(np.float64)
    rm, rv = _f(rm).astype(np.float64), _f(rv).astype(np.float64)
    if fp32:
        f = np.float32
        m1 = _f(_f(S1) / f(cnt))
        m2 = _f(_f(S2) / f(cnt))
        var = np.maximum(_f(m2 - _f(m1 * m1)), f(0)).astype(np.float64)
        mu = _f(_f(p) + m1).astype(np.float64)
        m1 = m1.astype(np.float64)
    else:
        m1, m2 = S1 / cnt, S2 / cnt
        var = np.maximum(m2 - m1 * m1, 0.0)
        mu = p + m1
    a, b = (m, 1 - m) if swap_m else (1 - m, m)
    if pivot_after:       # the pivot read after the running-mean update (the two alias: the pivot is running_mean)
        mu = _f(a * rm + b * mu).astype(np.float64) + m1
    invstd = 1.0 / (np.sqrt(var) + eps) if eps_outside else 1.0 / np.sqrt(var + eps)
    unb = var if biased_rv else var * cnt / (cnt - 1.0)
    return _f(mu), _f(invstd), _f(a * rm + b * mu), _f(a * rv + b * unb)


def emulate_apply(x, mean, invstd, gamma, beta, res=None, relu=False, drop_rows=None, drop_twice=False):
    """k_bn_apply in fp32, no contraction"""
    v = _f(_f(_f(_f(_f(x) - mean) * invstd) * gamma) + beta)
    if res is not None:
        v = _f(v + _f(res))
    if relu:
        v = np.maximum(v, np.float32(0))
    if drop_rows is not None:
        v = _f(v * drop_rows)
        if drop_twice:
            v = _f(v * drop_rows)
    return v


def emulate_bwd(dy, x, y, mean, invstd, gamma, drop_rows=None, relu=True, mask_ge=False, swap_sums=False, dres_unmasked=False):
    """k_colreduce over BnBwdOp + k_bn_bwd_apply in fp32, the mask [y > 0] read from the forward's output -> dx, dres, S0, S1"""
    M = x.shape[0]
    dy = _f(dy)
    g = np.where((y >= 0) if mask_ge else (y > 0), dy, np.float32(0)) if relu else dy.copy()
    if drop_rows is not None:
        g = _f(g * drop_rows)
    dres = (_f(dy * drop_rows) if drop_rows is not None else dy.copy()) if dres_unmasked else g
    xh = _f(_f(_f(x) - mean) * invstd)
    S0 = emu_colreduce(g)
    S1 = emu_colreduce(_f(g * xh))
    a, b = (S1, S0) if swap_sums else (S0, S1)
    m0, m1 = _f(a / M), _f(b / M)
    dx = _f(_f(_f(gamma) * invstd) * _f(_f(g - m0) - _f(xh * m1)))
    return dx, dres, S0, S1
