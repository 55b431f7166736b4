"""The direct implicit-GEMM kernel k_conv_igemm<TM, TN, WM, BF> (u2pl_amd/csrc/conv.hip) on its own: the planner and kernel choice
restated, a float64 reference and per-element bound for every entry point, a numpy fp32 emulation of the kernel's order with
switchable faults, and the table of tile / loop / gather / pitch edges -- shared by tests/test_igemm_cpu.py and
tests/test_gpu_igemm_bounds.py.  Not a conftest: imported by name.  Also the tile plan of the pre-split GEMMs (csrc/igemm_ws.hip
plan_igemm_ws) restated, for tests/test_ws_plan_cpu.py.

    Y[m][co] = sum over (r, s, ci) of X[gather(m, r, s)][ci] * W[co][r][s][ci]        K = R S Cin

Forward: gather o * stride - pad + r * dil.  Data gradient: the same kernel on dY with the transposed weights [Cin][R][S][Cout],
gather (i + pad - r * dil) >> log2(stride) with a divisibility test.  Batched GEMM: gridDim.z independent products.

Bound of each output, per arithmetic (EPS = 2^-24; cond: the same product on absolute values):
  fp32    (K + 2) EPS cond     the derived worst case of an fp32 sum of K products in any order (u2pl_conv_set_split(0): BF = 0, the fp32
          matrix instruction).  Its excess over the 64-unit cap is a record, not an assertion.
  six     A_REL EPS cond       BF = 3: three bf16 pieces carry every finite fp32 to 2^-24, the dropped products are <= 2^-23 |ab|; no
          floor; A_REL = 64 is the cap the project applies to every split arithmetic (split_bounds.py)
  bf16op  `six`, against the float64 product of the operands rounded to bf16 (round to nearest even): BF = 1, the products are exact
  bias    v = ref + bias, + EPS |v|
  eval BatchNorm (+ residual, ReLU)    s = gamma invstd, t = beta - mean s, pre = v s + t + res:
          |s| bound(v) + C_EPI EPS (|v s| + |mean s| + |beta| + |res|)      (test_eval_batchnorm_epilogue_meets_the_bound's form)
Where cond is 0 (every tap of the output outside the map) the bound is 0: the output is the bias, or exactly 0.

Fused statistics.  Block b of a launch (body: 128 rows each from row 0, slots 0 ..; tail: BM rows each from m_body, slots nblk_body ..)
writes S1[c] = sum t_m and S2[c] = sum t_m^2 over its valid rows, t_m = fl(acc_m + sh), sh = fl(bias - pivot) (k_conv_igemm: `const float
v = m < M ? acc[a][b][e] + sh : 0.f; s1 += v; s2 += v * v;`, then the lane halves and the WM wave rows added).  Against d_m = v_m - p in
float64 (v_m = ref_m + bias):
  a_m = |t_m - d_m| <= (1 + EPS) (P_m + EPS |bias - p|) + EPS |d_m|       P_m: the product bound of row m; one rounding of sh, one of the sum
  S1: rows - 1 additions in any order lose at most (rows - 1) EPS sum |t_m| (to first order; the 3 spare units cover the second-order
      terms of rows <= 128), so  E1 = sum a_m + (rows + 2) EPS sum (|d_m| + a_m)
  S2: |t_m^2 - d_m^2| <= a_m (2 |d_m| + a_m); the square is one more rounding (none where it is fused into the addition):
      E2 = sum a_m (2 |d_m| + a_m) + (rows + 2) EPS sum (|d_m| + a_m)^2
rows: the block's valid rows (the padded rows add exact zeros).  Nothing is fitted to a measured error.

Mutant (emulate(fault=...)) -> the kernel line it stands for:
  unmasked_rows        `mv[i] = m < M` of the loads together with `if (m < M)` of the store (mv alone only changes accumulator rows that are
                       never stored: the store guard is what makes the missing mask visible)
  no_parity            `((v & ((1 << log2div) - 1)) == 0)` of gather_coord
  no_upper_limit       `(q < lim)` of gather_coord
  swap_rs              `r = tap / g.S, s = tap - r * g.S` of load_chunk
  stride_as_dil        `g.step` handed to gather_coord (g.mul in its place)
  skip_last_odd_chunk  `if (kc + 1 < nk)` / `if (kc + 1 >= nk) break` taken as the loop's own condition: an odd last chunk is never multiplied
  stale_prefetch       `store_chunk(0, ra1, rb1)` storing ra0 (which holds chunk kc + 3) where chunk kc + 2 belongs
  bias_past_cout       `bias[cbase + j]` read one column further (the last column reads past Cout)
  store_past_cout      `cbase + j < g.Cout` of the stores (vector: `cbase + 3 < g.Cout`)
  ldy_ignored          `y + m * ldy`
  ldx_ignored          `ldxb = (int)ldx * 4`
  batch_stride_ignored `x += blockIdx.z * zx; w += blockIdx.z * zw; y += blockIdx.z * zy` (dense strides in their place)
  stats_rows_unmasked  `m < M ? acc[a][b][e] + sh : 0.f` (padded rows add sh)
  stats_tail_at_zero   `stats + (long)p.nblk_body * 2 * g.Cout` of run_igemm
  stats_without_bias   `bias ? bias[co] : 0.f` of sh
  relu_before_residual `if (epi.relu)` in front of `if (epi.res)`
  drop_piece           the a1 b0 product of the six
  bf16_once            split3_bf16's second and third piece of the gathered operand
"""
import collections
import os
import sys

import numpy as np
import torch
import torch.nn.functional as TF

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import split_bounds as SB  # noqa: E402
from test_split_fp32_cpu import bf16_rne, split3  # noqa: E402

F32 = np.float32
EPS, A_REL, C_EPI = SB.EPS, SB.A_REL, SB.C_EPI
BK = 32
NUM_CUS = 256
ARITHS = ("six", "fp32", "bf16op")
SENT = F32(-3.0e30)                     # what the tests put wherever the kernel must not write
FAULTS = ("unmasked_rows", "no_parity", "no_upper_limit", "swap_rs", "stride_as_dil", "skip_last_odd_chunk", "stale_prefetch",
          "bias_past_cout", "store_past_cout", "ldy_ignored", "ldx_ignored", "batch_stride_ignored", "stats_rows_unmasked",
          "stats_tail_at_zero", "stats_without_bias", "relu_before_residual", "drop_piece", "bf16_once")


def cdiv(a, b):
    return -(-a // b)


# ---- plan_igemm and run_igemm's kernel choice -----------------------------------------------------------------------------------------
Plan = collections.namedtuple("Plan", "m_body tail_tm tail_tn nblk_body nblk_tail")
Launch = collections.namedtuple("Launch", "TM TN WM BF BM BN m0 m1 slot")


def _atoi(s):
    s = s.strip()
    i, sign = 0, 1
    if s[:1] in ("+", "-"):
        sign, i = (-1 if s[0] == "-" else 1), 1
    j = i
    while j < len(s) and s[j].isdigit():
        j += 1
    return sign * int(s[i:j]) if j > i else 0


def _tail_cost(rows, cout, bm, bn, eff):
    return float(cdiv(cdiv(rows, bm) * cdiv(cout, bn), NUM_CUS)) * bm * bn / eff


def plan_igemm(M, Cout, split, tail=None, batch=1):
    """csrc/conv.hip plan_igemm.  split: u2pl_conv_get_split(); tail: the value of U2PL_IGEMM_TAIL (None or "": unset)"""
    if Cout <= 64:
        return Plan(M, 0, 0, cdiv(M, 128), 0)
    nt = cdiv(Cout, 128) * batch
    mtiles = cdiv(M, 128)
    body_tiles = min((mtiles * nt // NUM_CUS) * NUM_CUS // nt, mtiles)
    m_body = min(body_tiles * 128, M)
    nblk_body = cdiv(m_body, 128)
    t = M - m_body
    if t <= 0:
        return Plan(m_body, 0, 0, nblk_body, 0)
    c22, c12, c11 = (_tail_cost(t, Cout * batch, bm, bn, eff) for bm, bn, eff in ((128, 128, 1.0), (64, 128, 0.9), (64, 64, 0.8)))
    tm, tn = (2, 2) if (c22 <= c12 and c22 <= c11) else (1, 2) if c12 <= c11 else (1, 1)
    e = tail if tail else ("0" if split else None)
    if e and _atoi(e) >= 0:
        v = _atoi(e)
        if v == 0:
            return Plan(M, 0, 0, cdiv(M, 128), 0)
        tm, tn = {22: (2, 2), 12: (1, 2), 11: (1, 1), 14: (4, 1)}.get(v, (tm, tn))
    return Plan(m_body, tm, tn, nblk_body, cdiv(t, 128) if tm == 4 else cdiv(t, 64 * tm))


def _launch(TM, TN, WM, BF, m0, m1, slot):
    return Launch(TM, TN, WM, BF, 32 * TM * WM, 64 * TN, m0, m1, slot)


def run_igemm(M, Cout, split, bf16op=False, tail=None, waves=8, batch=1):
    """the launches of run_igemm in order (empty row ranges are not launched).  BF: 3 six products (split on), 1 bf16-rounded operands,
    0 the fp32 matrix instruction; waves: U2PL_IGEMM_WAVES (4 selects the <2, 2, 2> body for BF 0 and 3)"""
    p = plan_igemm(M, Cout, split, tail, batch)
    BF = 1 if bf16op else 3 if split else 0
    if Cout <= 64:
        out = [_launch(2, 1, 2, BF, 0, M, 0)]
    else:
        body = (2, 2, 2) if (waves == 4 and BF != 1) else (1, 2, 4)
        out = [_launch(*body, BF, 0, p.m_body, 0)]
        if p.nblk_tail:
            shape = (1, 1, 4) if p.tail_tm == 4 else (2, 2, 2) if p.tail_tm == 2 else (1, 2, 2) if p.tail_tn == 2 else (1, 1, 2)
            out.append(_launch(*shape, BF, p.m_body, M, p.nblk_body))
    return [l for l in out if l.m1 > l.m0]


def stat_blocks(launches):
    return sum(cdiv(l.m1 - l.m0, l.BM) for l in launches)


def shape_of(l):
    return "<%d, %d, %d, %d>" % (l.TM, l.TN, l.WM, l.BF)


# ---- plan_igemm_ws (csrc/igemm_ws.hip): the tile plan of the pre-split GEMMs ----------------------------------------------------------
WS_WIDE, WS_NARROW, WS_MIXED, WS_MIXED2 = 0, 1, 2, 3
WsPlan = collections.namedtuple("WsPlan", "kind wide narrow")


def plan_igemm_ws(M, K, Cout, batch, np_, narrow=None, mix2=0, fix2=2.0, persist=1):
    """u2pl_igemm_ws_plan.  np_: pieces per operand (3 six bf16 products, 2 split-fp16); narrow: the integer value of U2PL_WS_NARROW (None:
    unset), mix2: U2PL_WS_MIX2, fix2: U2PL_WS_FIX2, persist: u2pl_igemm_ws_set_persist.  Costs in units of one 32-deep chunk of a 128 x 256
    tile: a narrow tile takes 0.5 x 1.15 of it, a tile has a fixed cost of 4 (wide) or 2 (narrow) units, `fix2` times that for split-fp16;
    the mixed plan pays 2 more (8 as two launches) and must beat the wide plan by 3 %."""
    mt, nkc = cdiv(M, 128), K // BK
    ntw, ntn = cdiv(Cout, 256), cdiv(Cout, 128)
    tw, tn = mt * ntw * batch, mt * ntn * batch
    wide, nar = WsPlan(WS_WIDE, tw, 0), WsPlan(WS_NARROW, 0, tn)
    if Cout <= 128:
        return nar
    fix = 1.0 if np_ == 3 else fix2
    cw1, cn1 = nkc + 4.0 * fix, 0.5 * 1.15 * nkc + 2.0 * fix
    cw, cn = float(cdiv(tw, NUM_CUS)) * cw1, float(cdiv(tn, NUM_CUS)) * cn1
    if narrow == 0:
        return wide
    if narrow == 1:
        return nar if Cout <= 256 else wide
    full = tw // NUM_CUS * NUM_CUS
    rem = tw - full
    can_mix = narrow != 2 and persist and ntn == 2 * ntw and full > 0 and rem > 0 and 2 * rem <= NUM_CUS
    cm = float(full // NUM_CUS) * cw1 + cn1 + (8.0 if mix2 else 2.0) * fix if can_mix else 1e30
    if cm < 0.97 * cw and cm < cn:
        return WsPlan(WS_MIXED2 if mix2 else WS_MIXED, full, 2 * rem)
    return nar if cn < 0.97 * cw else wide


def ws_plan_sweep():
    """(M, K, Cout, batch) across every boundary of the model: Cout 128 / 129 (the narrow-only range), 256 / 257 (one or two wide column
    tiles; 257 .. 384 has three narrow ones: no mixing), 512; wide tile counts either side of a round (256) and of the largest mixable
    remainder (2 rem = 256 | 258); K from one chunk to 4608, with the chunk counts between which the mixed plan starts to win on 257 tiles:
    13 / 14 (np 3) and 26 / 27 (np 2) in one launch, 53 / 54 and 106 / 107 as two launches (U2PL_WS_MIX2)"""
    out = []
    for Cout in (65, 128, 129, 256, 257, 384, 385, 512, 513, 1024, 2048):
        ntw = cdiv(Cout, 256)
        for batch in (1, 16, 36):
            mts = set()
            for tw in (1, 128, 255, 256, 257, 300, 383, 384, 385, 511, 512, 513, 640, 641, 792, 1000):
                mts |= {max(1, tw // (ntw * batch)), cdiv(tw, ntw * batch)}
            for mt in sorted(mts):
                for K in (32, 256, 416, 448, 512, 832, 864, 1024, 1696, 1728, 2304, 3392, 3424, 4608):
                    out.append((mt * 128 - 5, K, Cout, batch))
    return out


# ---- geometry -------------------------------------------------------------------------------------------------------------------------
# ConvGeom of conv_geom.h with off_h = off_w; gather: (o * mul + off + tap * step) >> log2div
Geo = collections.namedtuple("Geo", "N Hin Win Cin Hout Wout Cout R S mul off step log2div")
# kind: fwd | dgrad.  N, H, W: the layer's input map; C: the GEMM's reduction channels (a multiple of 32: the layer's Cin forward, its
# Cout in the data gradient); the GEMM's column count (layer Cout forward, layer Cin in the data gradient) is chosen per run
Case = collections.namedtuple("Case", "name kind N H W C k stride pad dil")


def out_size(h, k, stride, pad, dil):
    return (h + 2 * pad - dil * (k - 1) - 1) // stride + 1


def geo(case, ncol):
    Ho, Wo = out_size(case.H, case.k, case.stride, case.pad, case.dil), out_size(case.W, case.k, case.stride, case.pad, case.dil)
    if case.kind == "fwd":
        return Geo(case.N, case.H, case.W, case.C, Ho, Wo, ncol, case.k, case.k, case.stride, -case.pad, case.dil, 0)
    return Geo(case.N, Ho, Wo, case.C, case.H, case.W, ncol, case.k, case.k, 1, case.pad, -case.dil, case.stride.bit_length() - 1)


def gemm_geo(M, K, Nn):
    return Geo(1, M, 1, K, M, 1, Nn, 1, 1, 1, 0, 1, 0)


def rows_out(g):
    return g.N * g.Hout * g.Wout


# ---- operands -------------------------------------------------------------------------------------------------------------------------
KINDS = ("relu_heavy_tail", "cancellation", "normal")


def operands(kind, pixels, C, ncol, taps, seed):
    """-> A rows [pixels][C], W [ncol][taps][C] float32 (the kinds of split_bounds.operands, and plain normal)"""
    if kind == "normal":
        rng = np.random.default_rng(seed)
        A, B = rng.standard_normal((pixels, C)), rng.standard_normal((C, ncol * taps)) / np.sqrt(C)
    else:
        A, B = SB.operands(kind, pixels, C, ncol * taps, seed)
    W = (np.asarray(B, dtype=np.float64).T.reshape(ncol, taps, C) / np.sqrt(taps))
    return np.ascontiguousarray(A, dtype=F32), np.ascontiguousarray(W, dtype=F32)


def pitched(a, ld, behind=0, fill=np.nan, shift=0):
    """rows [M][C] -> flat float32 [shift + (M + behind) ld]: `fill` in front, in the gaps and in the rows behind the last one"""
    M, C = a.shape
    b = np.full(shift + (M + behind) * ld, fill, dtype=F32)
    b[shift:].reshape(M + behind, ld)[:M, :C] = a
    return b


def unpitch(flat, M, C, ld, shift=0):
    return flat[shift:shift + M * ld].reshape(M, ld)[:, :C]


def outside_intact(flat, M, C, ld, shift=0, fill=SENT):
    """nothing outside the [M][C] output changed"""
    mask = np.ones(flat.shape, dtype=bool)
    mask[shift:shift + M * ld].reshape(M, ld)[:, :C] = False
    return bool((flat[mask].view(np.uint32) == F32(fill).reshape(1).view(np.uint32)[0]).all())


# ---- float64 reference and bounds -----------------------------------------------------------------------------------------------------
def product_ref(case, ncol, A, W, arith):
    """-> (ref, cond) float64 numpy [rows][ncol] by torch's convolution (forward) or its input gradient (data gradient)"""
    assert arith in ARITHS
    if arith == "bf16op":
        A, W = bf16_rne(A), bf16_rne(W)
    g = geo(case, ncol)
    a = torch.from_numpy(np.asarray(A, dtype=np.float64)).reshape(g.N, g.Hin, g.Win, g.Cin).permute(0, 3, 1, 2)
    w = torch.from_numpy(np.asarray(W, dtype=np.float64)).reshape(ncol, case.k, case.k, case.C)
    kw = dict(stride=case.stride, padding=case.pad, dilation=case.dil)
    if case.kind == "fwd":
        f = lambda a_, w_: TF.conv2d(a_, w_.permute(0, 3, 1, 2), **kw)                                         # noqa: E731
    else:
        f = lambda a_, w_: torch.nn.grad.conv2d_input((case.N, ncol, case.H, case.W), w_.permute(3, 0, 1, 2), a_, **kw)   # noqa: E731
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(-1, ncol).numpy()                                           # noqa: E731
    return rows(f(a, w)), rows(f(a.abs(), w.abs()))


def gemm_ref(X, W, arith):
    """X [batch][M][K], W [batch][Nn][K] -> (ref, cond) [batch][M][Nn]"""
    if arith == "bf16op":
        X, W = bf16_rne(X), bf16_rne(W)
    X, W = np.asarray(X, dtype=np.float64), np.asarray(W, dtype=np.float64)
    return np.einsum("zmk,znk->zmn", X, W), np.einsum("zmk,znk->zmn", np.abs(X), np.abs(W))


def product_bound(cond, K, arith):
    return (K + 2) * EPS * cond if arith == "fp32" else A_REL * EPS * cond


def cap_bound(cond):
    """the 64-unit cap alone (what the fp32 instruction's excess is RECORDED against)"""
    return A_REL * EPS * cond


def y_ref_bound(ref, cond, K, arith, bias=None):
    pb = product_bound(cond, K, arith)
    if bias is None:
        return ref, pb
    v = ref + np.asarray(bias, dtype=np.float64)
    return v, pb + EPS * np.abs(v)


def bnact_ref_bound(v, bv, mean, invstd, gamma, beta, res=None, relu=0):
    mean, invstd, gamma, beta = (np.asarray(t, dtype=np.float64) for t in (mean, invstd, gamma, beta))
    s = gamma * invstd
    r = 0.0 if res is None else np.asarray(res, dtype=np.float64)
    pre = v * s + (beta - mean * s) + r
    bound = np.abs(s) * bv + C_EPI * EPS * (np.abs(v * s) + np.abs(mean * s) + np.abs(beta) + np.abs(r))
    return (np.maximum(pre, 0.0) if relu else pre), bound


def stats_ref_bound(v, pb, bias, pivot, launches):
    """v [M][Cout] float64 (bias included), pb: the product bound of each element -> (ref, bound) [nblk][2][Cout] in the kernel's block
    order (module docstring)"""
    M, Cout = v.shape
    b = np.zeros(Cout) if bias is None else np.asarray(bias, dtype=np.float64)
    p = np.zeros(Cout) if pivot is None else np.asarray(pivot, dtype=np.float64)
    d = v - p
    a = (1 + EPS) * (pb + EPS * np.abs(b - p)) + EPS * np.abs(d)
    n = stat_blocks(launches)
    ref, bound = np.zeros((n, 2, Cout)), np.zeros((n, 2, Cout))
    for l in launches:
        for bx in range(cdiv(l.m1 - l.m0, l.BM)):
            r0, r1 = l.m0 + bx * l.BM, min(l.m1, l.m0 + (bx + 1) * l.BM)
            dd, aa = d[r0:r1], a[r0:r1]
            ref[l.slot + bx, 0], ref[l.slot + bx, 1] = dd.sum(0), (dd * dd).sum(0)
            t = np.abs(dd) + aa
            bound[l.slot + bx, 0] = aa.sum(0) + (r1 - r0 + 2) * EPS * t.sum(0)
            bound[l.slot + bx, 1] = (aa * (2 * np.abs(dd) + aa)).sum(0) + (r1 - r0 + 2) * EPS * (t * t).sum(0)
    return ref, bound


def excess(got, ref, bound):
    return SB.excess(np.asarray(got, dtype=np.float64), np.asarray(ref), np.asarray(bound))


# ---- the kernel's order in numpy fp32 -------------------------------------------------------------------------------------------------
def gather_coord(base, tap, step, log2div, lim, fault=None):
    v = base + tap * step
    q = v >> log2div
    ok = v >= 0
    if fault != "no_parity":
        ok = ok & ((v & ((1 << log2div) - 1)) == 0)
    if fault != "no_upper_limit":
        ok = ok & (q < lim)
    return ok, np.where(ok, q, 0)


def k_schedule(nk, single, fault=None):
    """the chunk multiplied at each step of the K loop: double-buffered with guarded loads (BF 0 / 1), or one buffer with clamped loads
    (BF 3).  Faithful: 0 .. nk - 1 in order."""
    used = []
    reg0 = 1 if nk > 1 else 0
    reg1 = 2 if nk > 2 else None
    nloop = nk - nk % 2 if fault == "skip_last_odd_chunk" else nk
    stale = fault == "stale_prefetch"
    if single:
        cur = 0
        for kc in range(0, nloop, 2):
            used.append(cur)
            cur, reg0 = reg0, min(kc + 3, nk - 1)
            if kc + 1 >= nk:
                break
            used.append(cur)
            cur, reg1 = (reg0 if stale else reg1), min(kc + 4, nk - 1)
    else:
        lds = {0: 0}
        for kc in range(0, nloop, 2):
            used.append(lds[0])
            if kc + 1 < nk:
                lds[1] = reg0
            if kc + 3 < nk:
                reg0 = kc + 3
            if kc + 1 < nk:
                used.append(lds[1])
                if kc + 2 < nk:
                    lds[0] = reg0 if stale else reg1
                if kc + 4 < nk:
                    reg1 = kc + 4
    assert None not in used
    return used


def _read(buf, off, C, ok, lim):
    """rows of C floats at float offsets `off` of a flat buffer, as the raw-buffer descriptor of `lim` floats returns them: zero where not
    ok and at or past lim (NaN past the allocation itself)"""
    buf = np.concatenate([np.asarray(buf, dtype=F32), F32([np.nan])])
    idx = off[..., None] + np.arange(C)
    good = ok[..., None] & (idx >= 0) & (idx < lim)
    return np.where(good, buf[np.clip(idx, 0, len(buf) - 1)], F32(0))


def _tile_sum(T, TM, WM):
    """T [blocks][BM][cols] float32 -> [blocks][cols]: per wave row wm and lane half lh the TM x 16 register values in (a, e) order (rows
    wm 32 TM + a 32 + (e & 3) + 8 (e >> 2) + 4 lh), the halves added, the WM wave rows added in order"""
    tot = None
    for wm in range(WM):
        halves = []
        for lh in range(2):
            s = np.zeros((T.shape[0], T.shape[2]), dtype=F32)
            for a in range(TM):
                for e in range(16):
                    s = s + T[:, wm * 32 * TM + a * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh]
            halves.append(s)
        blk = halves[0] + halves[1]
        tot = blk if tot is None else tot + blk
    return tot


SIX_ORDER = [(2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0)]
Epi = collections.namedtuple("Epi", "mean invstd gamma beta res ldr relu")


def emulate(x, ldx, w, g, launches, y, ldy, yshift=0, bias=None, want_stats=False, pivot=None, batch=1, zx=0, zw=0, zy=0, epi=None,
            fault=None):
    """x, w: flat float32 buffers; y: the flat output buffer as handed to the kernel (a copy is written and returned), the output starting
    `yshift` floats into it; g: Geo; launches: run_igemm(...).  -> (y, stats [nblk][2][Cout] or None, info); info["scalar"]: the stores
    took the scalar path.  The products of a k block (2 for the fp32 instruction, 16 for bf16) exact in float64, added to an fp32
    accumulator; six: the piece products in the kernel's order."""
    assert fault is None or fault in FAULTS
    x, w = np.asarray(x, dtype=F32), np.asarray(w, dtype=F32)
    y = np.array(y, dtype=F32)
    M, K = rows_out(g), g.R * g.S * g.Cin
    nk, cpt = K // BK, g.Cin // BK
    assert g.Cin % BK == 0
    xlim, wlim = (g.N * g.Hin * g.Win - 1) * ldx + g.Cin, g.Cout * K
    ldxe = g.Cin if fault == "ldx_ignored" else ldx
    ldye = g.Cout if fault == "ldy_ignored" else ldy
    if fault == "batch_stride_ignored":
        zx, zw, zy = g.N * g.Hin * g.Win * ldx, g.Cout * K, M * ldy
    step = g.mul if fault == "stride_as_dil" else g.step
    nstat = stat_blocks(launches)
    stats = np.full((nstat, 2, g.Cout), np.nan, dtype=F32) if want_stats else None
    vec_ok = ldy % 4 == 0 and yshift % 4 == 0
    info = {"scalar": (not vec_ok) or g.Cout % 4 != 0, "shapes": [shape_of(l) for l in launches]}
    ybig = np.concatenate([y, np.full(256 * (ldy + 1) + 256, SENT, dtype=F32)])       # room for what a missing guard writes
    for l in launches:
        nrb, ncb = cdiv(l.m1 - l.m0, l.BM), cdiv(g.Cout, l.BN)
        m = l.m0 + np.arange(nrb * l.BM)
        rowv = m < l.m1
        mv = np.ones_like(rowv) if fault == "unmasked_rows" else rowv
        mm = np.where(mv, m, 0)
        t = mm // g.Wout
        wo, n = mm - t * g.Wout, t // g.Hout
        ho = t - n * g.Hout
        bh, bw, nb = ho * g.mul + g.off, wo * g.mul + g.off, n * g.Hin * g.Win
        co = np.arange(ncb * l.BN)
        cv = co < g.Cout
        for z in range(batch):
            xz, wz = x[z * zx:], w[z * zw:]
            A = np.zeros((len(m), K), dtype=F32)
            for kc in range(nk):
                tap = kc // cpt
                c0 = (kc - tap * cpt) * BK
                r, s = tap // g.S, tap - (tap // g.S) * g.S
                if fault == "swap_rs":
                    r, s = s, r
                okh, ih = gather_coord(bh, r, step, g.log2div, g.Hin, fault)
                okw, iw = gather_coord(bw, s, step, g.log2div, g.Win, fault)
                A[:, kc * BK:(kc + 1) * BK] = _read(xz, (nb + ih * g.Win + iw) * ldxe + c0, BK, mv & okh & okw, xlim)
            B = _read(wz, co * K, K, cv, wlim)
            with np.errstate(invalid="ignore", over="ignore"):
                if l.BF == 3:
                    pa, pb = split3(A)[:3], split3(B)[:3]
                    if fault == "bf16_once":
                        pa = (bf16_rne(A), np.zeros_like(A), np.zeros_like(A))
                    order = [o for o in SIX_ORDER if not (fault == "drop_piece" and o == (1, 0))]
                elif l.BF == 1:
                    pa, pb, order = (bf16_rne(A),), (bf16_rne(B),), [(0, 0)]
                else:
                    pa, pb, order = (A,), (B,), [(0, 0)]
                pa, pb = [q.astype(np.float64) for q in pa], [q.astype(np.float64) for q in pb]
                acc = np.zeros((len(m), len(co)), dtype=F32)
                for kc in k_schedule(nk, l.BF == 3, fault):
                    if l.BF == 0:       # lane half h supplies k = 8 gk + 4 h + j at step j: one instruction adds two products
                        blocks = [[kc * BK + 8 * gk + j, kc * BK + 8 * gk + 4 + j] for gk in range(BK // 8) for j in range(4)]
                    else:
                        blocks = [list(range(kc * BK + 16 * gk, kc * BK + 16 * gk + 16)) for gk in range(BK // 16)]
                    for ks in blocks:
                        for ia, ib in order:
                            acc = (acc.astype(np.float64) + pa[ia][:, ks] @ pb[ib][:, ks].T).astype(F32)
                # epilogue
                v = acc
                if bias is not None:
                    bx = np.concatenate([np.asarray(bias, dtype=F32), np.full(len(co) + 1, np.nan, dtype=F32)])
                    bvec = bx[co + 1] if fault == "bias_past_cout" else np.where(cv, bx[np.minimum(co, g.Cout - 1)], F32(0))
                    v = (acc + bvec[None]).astype(F32)
                if epi is not None:
                    cc = np.minimum(co, g.Cout - 1)
                    mu, isd, ga, be = (np.asarray(q, dtype=F32)[cc][None] for q in (epi.mean, epi.invstd, epi.gamma, epi.beta))
                    e_ = ((((v - mu).astype(F32) * isd).astype(F32) * ga).astype(F32) + be).astype(F32)
                    if epi.relu and fault == "relu_before_residual":
                        e_ = np.maximum(e_, F32(0))
                    if epi.res is not None:
                        rv = _read(epi.res, np.where(rowv, m, 0) * epi.ldr, len(co), rowv, 1 << 40)
                        e_ = (e_ + rv).astype(F32)
                    if epi.relu and fault != "relu_before_residual":
                        e_ = np.maximum(e_, F32(0))
                    v = np.where(rowv[:, None] & cv[None], e_, v)
                srow = np.ones_like(rowv) if fault == "unmasked_rows" else rowv
                scol = np.ones_like(cv) if fault == "store_past_cout" else cv
                idx = yshift + z * zy + m[:, None] * ldye + co[None]
                sel = srow[:, None] & scol[None] & (idx < len(ybig))
                ybig[idx[sel]] = v[sel]
                if want_stats and z == 0:
                    bz = np.zeros(len(co), dtype=F32) if (bias is None or fault == "stats_without_bias") else np.where(
                        cv, np.asarray(bias, dtype=F32)[np.minimum(co, g.Cout - 1)], F32(0))
                    pz = np.zeros(len(co), dtype=F32) if pivot is None else np.where(cv, np.asarray(pivot, dtype=F32)[np.minimum(co, g.Cout - 1)], F32(0))
                    sh = (bz - pz).astype(F32)
                    T = (acc + sh[None]).astype(F32)
                    if fault != "stats_rows_unmasked":
                        T = np.where(rowv[:, None], T, F32(0))
                    T = T.reshape(nrb, l.BM, len(co))
                    s1, s2 = _tile_sum(T, l.TM, l.WM), _tile_sum((T * T).astype(F32), l.TM, l.WM)
                    slot = 0 if (fault == "stats_tail_at_zero") else l.slot
                    stats[slot:slot + nrb, 0], stats[slot:slot + nrb, 1] = s1[:, :g.Cout], s2[:, :g.Cout]
    return ybig[:len(y)], stats, info


# ---- the table of edges ---------------------------------------------------------------------------------------------------------------
# tile shape (TM, TN, WM) -> (the U2PL_IGEMM_TAIL that forces it on a map of less than a round, BM, BN, the column counts of its edges)
SHAPES = collections.OrderedDict([
    ((2, 1, 2), (None, 128, 64, (20, 64, 19, 21))),         # Cout <= 64: the single launch, whatever the variable says
    ((1, 2, 4), ("0", 128, 128, (68, 128, 132))),           # the 8-wave body forced onto small maps
    ((2, 2, 2), ("22", 128, 128, (68, 128, 132))),
    ((1, 1, 4), ("14", 128, 64, (68, 128, 132))),
    ((1, 2, 2), ("12", 64, 128, (68, 128, 132))),
    ((1, 1, 2), ("11", 64, 64, (68, 128, 132))),
])
TAILS = (None, "0", "11", "12", "22", "14", "-1")


def _factor(M):
    """M = N H W with N > 1 where M allows it (a tile then spans images) and H as near to W as it goes"""
    N = next((q for q in (2, 3, 5, 7) if M % q == 0 and M > q), 1)
    P = M // N
    H = max(h for h in range(1, int(P ** 0.5) + 1) if P % h == 0)
    return N, H, P // H


def row_case(M):
    N, H, W = _factor(M)
    return Case("rows%d" % M, "fwd", N, H, W, 32, 3, 1, 1, 1)


KLOOP = [Case("nk%d" % q, "fwd", 2, 5, 7, 32 * q, 1, 1, 0, 1) for q in (1, 2, 3, 4, 5)] + [
    Case("k3x3_c32", "fwd", 2, 5, 7, 32, 3, 1, 1, 1), Case("k3x3_c64", "fwd", 2, 5, 7, 64, 3, 1, 1, 1)]
GATHER = [
    Case("pad1", "fwd", 2, 5, 7, 32, 3, 1, 1, 1), Case("dil2", "fwd", 2, 5, 7, 32, 3, 1, 2, 2), Case("dil6_5x7", "fwd", 2, 5, 7, 32, 3, 1, 6, 6),
    Case("s2_odd", "fwd", 2, 9, 7, 32, 3, 2, 1, 1), Case("s2_even", "fwd", 2, 8, 6, 32, 3, 2, 1, 1), Case("pw_s2", "fwd", 2, 9, 7, 32, 1, 2, 0, 1),
    Case("s4", "fwd", 2, 9, 11, 32, 3, 4, 1, 1),
    Case("d_3x3", "dgrad", 2, 5, 7, 32, 3, 1, 2, 2), Case("d_s2_3x3", "dgrad", 2, 9, 7, 32, 3, 2, 1, 1), Case("d_s2_3x3_even", "dgrad", 2, 8, 6, 32, 3, 2, 1, 1),
    Case("d_s2_1x1", "dgrad", 2, 9, 7, 32, 1, 2, 0, 1), Case("d_s4", "dgrad", 2, 9, 11, 32, 3, 4, 1, 1),
]
BODY_TAIL = Case("body_tail", "fwd", 1, 65, 65, 32, 1, 1, 0, 1)
CASES = {c.name: c for c in KLOOP + GATHER + [BODY_TAIL]}

# one run of the table: a case, the GEMM's column count, the tile shape it is forced onto and how the buffers are laid out
Run = collections.namedtuple("Run", "case ncol shape ldx_extra ldy_extra yshift bias kind")


def _run(case, ncol, shape, ldx_extra=0, ldy_extra=0, yshift=0, bias=False, kind="relu_heavy_tail"):
    return Run(case, ncol, shape, ldx_extra, ldy_extra, yshift, bias, kind)


def run_id(r):
    return "%s-%d-%d%d%d%s%s%s%s" % ((r.case.name, r.ncol) + (r.shape or (0, 0, 0)) + ("-ldx%d" % r.ldx_extra if r.ldx_extra else "", "-ldy%d" % r.ldy_extra if r.ldy_extra else "",
                                     "-shift%d" % r.yshift if r.yshift else "", "-bias" if r.bias else ""))


def runs():
    out = []
    for i, (shape, (_, BM, BN, couts)) in enumerate(SHAPES.items()):
        for j, M in enumerate((1, BM - 1, BM, BM + 1, 2 * BM + 5)):                 # rows: a 3x3 whose tiles span images
            out.append(_run(row_case(M), couts[0], shape, bias=bool(j & 1), kind=KINDS[(i + j) % 3]))
        for j, ncol in enumerate(couts):                                            # columns, at one row past a tile
            out.append(_run(row_case(BM + 1)._replace(name="cols%d" % (BM + 1), C=64, k=1, pad=0), ncol, shape, bias=True, kind=KINDS[j % 3]))
    for shape, ncol in (((2, 1, 2), 20), ((1, 2, 4), 68), ((1, 1, 2), 132)):
        for j, c in enumerate(KLOOP):                                               # the K loop
            out.append(_run(c, ncol, shape, kind=KINDS[j % 3]))
    for shape, ncol in (((2, 1, 2), 20), ((1, 2, 2), 68)):
        for j, c in enumerate(GATHER):                                              # the gather
            out.append(_run(c, ncol, shape, bias=bool(j & 1) and c.kind == "fwd", kind=KINDS[j % 3]))      # (a data gradient has no bias)
    for shape, ncol in (((2, 1, 2), 64), ((1, 2, 4), 68), ((1, 1, 2), 128)):       # the pitch
        out.append(_run(CASES["pad1"], ncol, shape, ldx_extra=8, ldy_extra=8, bias=True))
        out.append(_run(CASES["pad1"], ncol, shape, ldx_extra=4, ldy_extra=3, bias=True, kind="cancellation"))      # ldy % 4 != 0: scalar stores
        out.append(_run(CASES["d_s2_3x3"], ncol, shape, ldx_extra=40, ldy_extra=24, kind="normal"))
        out.append(_run(CASES["nk3"], ncol, shape, yshift=1, bias=True))                                              # y one float into its allocation
    return out


BODY_TAIL_RUN = _run(BODY_TAIL, 1024, None, bias=True, ldy_extra=4)
# (arithmetic, split, U2PL_IGEMM_TAIL) under which the body + tail case gives both launches: the planner's own choice with the fp32
# instruction; -1 (the planner's choice) where the split switch is on, whose default is no tail
BODY_TAIL_STATES = (("fp32", 0, None), ("six", 1, "-1"), ("bf16op", 1, "-1"))
BATCHED = [(batch, 70, K, Nn) for batch in (16, 36) for K in (32, 96) for Nn in (20, 68)]


def state_of(arith):
    """-> (split, bf16op) of an arithmetic"""
    return {"six": (1, False), "fp32": (0, False), "bf16op": (1, True)}[arith]


def run_launches(r, arith, tail="table", waves=8):
    split, bf = state_of(arith)
    if tail == "table":
        tail = SHAPES[r.shape][0] if r.shape else None
    return run_igemm(rows_out(geo(r.case, r.ncol)), r.ncol, split, bf, tail, waves)


def run_data(r, seed=None):
    """-> dict: g, A, W (GEMM operands), bias, x / y flat buffers and pitches"""
    g = geo(r.case, r.ncol)
    seed = sum(map(ord, run_id(r))) if seed is None else seed
    A, W = operands(r.kind, g.N * g.Hin * g.Win, r.case.C, r.ncol, r.case.k ** 2, seed)
    bias = (np.random.default_rng(seed + 1).standard_normal(r.ncol) * 0.5).astype(F32) if r.bias else None
    ldx, ldy = r.case.C + r.ldx_extra, r.ncol + r.ldy_extra
    M = rows_out(g)
    return dict(g=g, A=A, W=W, bias=bias, ldx=ldx, ldy=ldy, M=M, x=pitched(A, ldx, behind=1), y=np.full(r.yshift + (M + 3) * ldy, SENT, dtype=F32))


def bn_params(ncol, M, ldr_extra, seed, with_res=True, relu=1):
    """eval-BatchNorm epilogue operands -> Epi (numpy; res flat [M][ncol + ldr_extra] with NaN in the gaps, or None)"""
    rng = np.random.default_rng(seed)
    mean, invstd = (rng.standard_normal(ncol) * 0.2).astype(F32), (1.0 / np.sqrt(rng.random(ncol) * 1.5 + 0.5)).astype(F32)
    gamma, beta = (rng.standard_normal(ncol) * 0.2 + 1.0).astype(F32), (rng.standard_normal(ncol) * 0.2).astype(F32)
    res = pitched(rng.standard_normal((M, ncol)).astype(F32), ncol + ldr_extra) if with_res else None
    return Epi(mean, invstd, gamma, beta, res, ncol + ldr_extra, relu)


def held(d, r, yflat, ref, bound):
    """excess of the [M][ncol] output inside a flat buffer; inf where anything outside the output changed"""
    if not outside_intact(yflat, d["M"], r.ncol, d["ldy"], r.yshift):
        return float("inf")
    return excess(unpitch(yflat, d["M"], r.ncol, d["ldy"], r.yshift), ref, bound)
