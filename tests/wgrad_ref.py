"""The weight-gradient kernels on their own: slab planners, kernel choice, float64 reference, per-arithmetic bound, a numpy fp32
emulation of the kernels' order with switchable faults, and the table of dispatch edges -- shared by tests/test_wgrad_cpu.py and
tests/test_gpu_wgrad_bounds.py.  Not a conftest: imported by name.

    dW[co][r][s][ci] = sum over pixels m of dY[m][co] * X[gather(m, r, s)][ci]

Kernels (u2pl_amd/csrc): k_wgrad_tr<TN, PW, NP> (wgrad_tr.hip; NP = 2 split-fp16 `h`, NP = 3 six bf16 piece products),
k_conv_wgrad_bf16<TM, TN, SP> (conv.hip; SP = 3 six products, SP = 1 bf16-rounded operands `bf16op`), k_conv_wgrad<TM, TN, WM>
(conv.hip; the fp32 matrix instruction), k_wgrad_reduce (conv.hip; slabs added in order).

Bound of each output element, per arithmetic (EPS = 2^-24; cond: the same gradient on absolute values):

  h       A_REL EPS cond + FLOOR (g_max (1 * |x|) + x_max (|gy| * 1))      split_bounds.conv_dw_bound's expression; the two maxima of
          the floor are the values HANDED TO THE KERNEL (an upper bound of the true maximum widens the fp16 subnormal spacing with it)
  six     A_REL EPS cond      three bf16 pieces carry every finite fp32 to 2^-24, the dropped products are <= 2^-23 |ab|: 3 units of
          representation, no floor; A_REL = 64 is the cap the project applies to every split arithmetic (split_bounds.py)
  fp32    (M + 2) EPS cond    M = N Ho Wo: the derived worst case of an fp32 sum of M products in any order (test_gpu_gconv.py; the
          slab sums fit it).  Its excess over the 64-unit cap is a record, not an assertion.
  bf16op  `six`, against the float64 product of the operands rounded to bf16 (round to nearest even): the products are then exact
  accumulate = 1: one more rounding, EPS (|previous| + |ref|)

Where cond is 0 (a tap outside the map for every pixel) the bound is 0: the output must be exactly 0.

Batched form (Winograd components): per component z and slab s the product dY_z[rows of s]^T X_z[rows of s]; slab layout
[nsplit][Cout][batch][Cin].

Mutant (emulate(fault=...)) -> the kernel line it stands for (all three kernels share the guards; names as in k_wgrad_tr):
  unmasked_rows     `mv` in row_offsets / load_chunk (`dyo = mv ? ... : OOB_OFF`, `okb = mv & okh & okw`)
  skip_odd_tail     `if (kc < nk) chunk(C0{})` behind the two-chunk loop of k_wgrad_tr
  store_ci_past     `if (ci >= g.Cin) continue` of the slab store (`ci < g.Cin`)
  store_co_past     `if (co < g.Cout) out[...] = ...` of the slab store
  no_accumulate     `accumulate ? ((const float4*)dw)[i] : 0` of k_wgrad_reduce
  drop_last_slab    the remainder loop `for (; z < nsplit; ++z)` of k_wgrad_reduce / gridDim.z = nsplit
  pitch_ignored     `lddyb = lddy * 4`, `ldxb = ldx * 4`
  swap_rs           `tr = tap / g.S, ts_ = tap - tr * g.S` handed to gather_coord
  stride_as_dil     `g.step` in gather_coord(ho * g.mul + g.off_h, tr, g.step, ...)
  scale_back_dy     `ldexpf(acc, -(e_dy + e_x))`
  amax_shard0       amax_read's maximum over the 64 shards
  drop_piece        QA / QB of do_mfma (the a1 b0 product)
  pass_bf16_once    split3_bf16's second and third piece of dY
"""
import collections
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import split_bounds as SB  # noqa: E402
from test_split_fp32_cpu import bf16_rne, split3  # noqa: E402

F32 = np.float32
EPS, A_REL, FLOOR = SB.EPS, SB.A_REL, SB.FLOOR
BK = 32
AMAX_SHARDS, AMAX_STRIDE = 64, 32
ARITHS = ("h", "six", "fp32", "bf16op")
FAULTS = ("drop_last_slab", "skip_odd_tail", "unmasked_rows", "pitch_ignored", "swap_rs", "stride_as_dil", "store_ci_past",
          "store_co_past", "no_accumulate", "scale_back_dy", "amax_shard0", "drop_piece", "pass_bf16_once")


def cdiv(a, b):
    return -(-a // b)


# ---- the two slab planners and the kernel choice ----------------------------------------------------------------------------------
def _finish(nchunks, want):
    cps = cdiv(nchunks, want)
    nsplit = cdiv(nchunks, cps)
    return nsplit, cps, nchunks - (nsplit - 1) * cps


def wgrad_tr_plan(M, Cin, Cout, taps, bn=0):
    """csrc/wgrad_tr.hip wgrad_tr_plan -> (ctiles, nsplit, cps, chunks in the last slab); bn: a forced tile width (U2PL_WT_BN)"""
    nchunks = cdiv(M, BK)
    bn = bn if bn in (128, 256) else (256 if Cin > 128 else 128)
    ctiles = cdiv(Cin, bn)
    tiles = cdiv(Cout, 128) * ctiles * taps
    best, bestc = 1, 1e30
    maxs = max(nchunks // 6, 1)
    for s in range(1, min(maxs, 96) + 1):
        c = cdiv(nchunks, s)
        if cdiv(nchunks, c) != s:
            continue
        cost = float(cdiv(tiles * s, 256)) * (c + 5.0) + 0.15 * s
        if cost < bestc:
            best, bestc = s, cost
    return (ctiles,) + _finish(nchunks, best)


def wgrad_plan(M, Cin, Cout, taps):
    """csrc/conv.hip wgrad_plan with its callers' tile choice -> (ctiles, nsplit, cps, chunks in the last slab)"""
    nchunks = cdiv(M, BK)
    BM, BN = (128 if Cout > 64 else 64), (128 if Cin > 64 else 64)
    ctiles = cdiv(Cin, BN)
    tiles = cdiv(Cout, BM) * ctiles * taps
    want = max(1, min(cdiv(1024, tiles), (nchunks + 7) // 8))
    return (ctiles,) + _finish(nchunks, want)


Choice = collections.namedtuple("Choice", "family BM BN PW NP tmpl")


def tr_eligible(Cin, Cout, tr):
    return bool(tr) and Cin >= 128 and Cout >= 128 and Cin % 4 == 0 and Cout % 4 == 0


def kernel_choice(Cin, Cout, split, tr, h, pointwise=False, bf16op=False, bn=0):
    """the kernel a weight gradient runs on, as the entry points of conv.hip decide it: split = u2pl_conv_set_split, tr =
    u2pl_wgrad_set_tr, h = the `_h_` entry point; pointwise: identity gather (1x1, stride 1, no padding; every batched call).
    NP: pieces per operand (3 six products, 2 split-fp16, 1 fp32 or bf16op)."""
    BM, BN = (128 if Cout > 64 else 64), (128 if Cin > 64 else 64)
    if bf16op:
        return Choice("k_conv_wgrad_bf16", BM, BN, False, 1, "<%d, %d, 1>" % (BM // 64, BN // 64))
    if h and not (split and tr_eligible(Cin, Cout, tr)):
        raise ValueError("the h form serves only eligible layers under both switches")
    if split and tr_eligible(Cin, Cout, tr):
        bn = bn if bn in (128, 256) else (256 if Cin > 128 else 128)
        return Choice("k_wgrad_tr", 128, bn, bool(pointwise), 2 if h else 3, "<%d, %s, %d>" % (bn // 128, str(bool(pointwise)).lower(), 2 if h else 3))
    if split:
        return Choice("k_conv_wgrad_bf16", BM, BN, False, 3, "<%d, %d, 3>" % (BM // 64, BN // 64))
    if BM == 128 and BN == 128:
        return Choice("k_conv_wgrad", BM, BN, False, 1, "<1, 2, 4>")
    return Choice("k_conv_wgrad", BM, BN, False, 1, "<%d, %d, 2>" % (BM // 64, BN // 64))


def plan_for(choice, M, Cin, Cout, taps):
    if choice.family == "k_wgrad_tr":
        return wgrad_tr_plan(M, Cin, Cout, taps, choice.BN)
    return wgrad_plan(M, Cin, Cout, taps)


# ---- geometry -------------------------------------------------------------------------------------------------------------------------
# gather: input coordinate = o * mul + off + tap * step (conv_geom.h); zdy / zx: floats between the components of a batched call
Geo = collections.namedtuple("Geo", "N Hin Win Cin Hout Wout Cout R S mul off step zdy zx")


def out_size(h, k, stride, pad, dil):
    return (h + 2 * pad - dil * (k - 1) - 1) // stride + 1


def conv_geo(N, H, W, Cin, Cout, k, stride, dil):
    """a k x k layer with `same` padding at stride 1 (pad = dil * (k // 2)) -> (Geo, pad)"""
    pad = dil * (k // 2)
    return Geo(N, H, W, Cin, out_size(H, k, stride, pad, dil), out_size(W, k, stride, pad, dil), Cout, k, k, stride, -pad, dil, 0, 0), pad


def batched_geo(M, Cin, Cout, batch, zdy, zx):
    return Geo(1, M, 1, Cin, M, 1, Cout, batch, 1, 1, 0, 0, zdy, zx)


def is_pointwise(g):
    return g.mul == 1 and g.off == 0 and g.Hin == g.Hout and g.Win == g.Wout and (g.step == 0 or g.R * g.S == 1)


# ---- operands -------------------------------------------------------------------------------------------------------------------------
def rows(kind, M, C, seed):
    """float32 [M][C]: split_bounds.operands' activation operand (`six_decade_rows`: a gradient, `relu_heavy_tail`: an activation)"""
    return SB.operands(kind, M, C + (C & 1), 1, seed)[0][:, :C].copy()


def nchw(a, N, H, W):
    """rows [N H W][C] -> torch [N][C][H][W]"""
    return torch.from_numpy(np.array(a, dtype=F32)).reshape(N, H, W, -1).permute(0, 3, 1, 2)


def pitched(a, ld, behind=3, fill=np.nan):
    """rows [M][C] -> flat float32 [(M + behind) ld]: `fill` in the gap and in the rows behind the last pixel"""
    M, C = a.shape
    b = np.full((M + behind, ld), fill, dtype=F32)
    b[:M, :C] = a
    return b.reshape(-1)


def amax_obj(value, shard=None):
    """the amax object as float32 words: `value` in every shard, or in `shard` alone with zeros elsewhere"""
    o = np.zeros(AMAX_SHARDS * AMAX_STRIDE, dtype=F32)
    if shard is None:
        o[::AMAX_STRIDE] = value
    else:
        o[shard * AMAX_STRIDE] = value
    return o


def amax_value(obj, shard0_only=False):
    bits = np.asarray(obj, dtype=F32).view(np.uint32)[::AMAX_STRIDE][:AMAX_SHARDS]
    return (bits[:1] if shard0_only else bits).max().reshape(1).view(F32)[0]


# ---- float64 reference and bound ------------------------------------------------------------------------------------------------------
def dw_ref(gy, x, ksize, stride=1, pad=0, dil=1, g_max=None, x_max=None, arith="h", prev=None):
    """gy [N][Cout][Ho][Wo], x [N][Cin][H][W] float32 -> (ref64, bound) as torch [Cout][R][S][Cin] (the kernels' layout).
    g_max / x_max: the maxima handed to the `h` kernel (default: the true ones); prev: the previous dw of accumulate = 1"""
    assert arith in ARITHS
    gy, x = gy.detach().cpu().float(), x.detach().cpu().float()
    if arith == "bf16op":
        gy, x = (torch.from_numpy(bf16_rne(t.contiguous().numpy())) for t in (gy, x))
    gy, x = gy.double(), x.double()
    ga, xa = gy.abs(), x.abs()
    shape = (gy.shape[1], x.shape[1]) + tuple(ksize)

    def c(g_, x_):
        return torch.nn.grad.conv2d_weight(x_, shape, g_, stride=stride, padding=pad, dilation=dil).permute(0, 2, 3, 1).contiguous()
    ref, cond = c(gy, x), c(ga, xa)
    if arith == "h":
        g_max = float(ga.max()) if g_max is None else float(g_max)
        x_max = float(xa.max()) if x_max is None else float(x_max)
        bound = A_REL * EPS * cond + FLOOR * (g_max * c(torch.ones_like(gy), xa) + x_max * c(ga, torch.ones_like(x)))
    elif arith == "fp32":
        bound = (gy.shape[0] * gy.shape[2] * gy.shape[3] + 2) * EPS * cond
    else:
        bound = A_REL * EPS * cond
    if prev is not None:
        pv = torch.as_tensor(np.asarray(prev, dtype=np.float64)).reshape(ref.shape)
        bound = bound + EPS * (pv.abs() + ref.abs())
        ref = pv + ref
    return ref, bound


def cap_bound(gy, x, ksize, stride=1, pad=0, dil=1):
    """the 64-unit cap A_REL EPS cond alone (what the fp32 kernels' excess is RECORDED against)"""
    return dw_ref(gy, x, ksize, stride, pad, dil, arith="six")[1]


def batched_ref(dY, X, M, batch, nsplit, cps, a_max=None, b_max=None, arith="h"):
    """dY [batch][M][Cout], X [batch][M][Cin] float32 -> (ref64, bound) [nsplit][Cout][batch][Cin]: slab s holds, per component z,
    dY_z[rows of slab s]^T X_z[rows of slab s]; the bound is split_bounds.gemm_bound with the maxima handed to the kernel (`h`) or
    its relative part alone (`six`)"""
    dY, X = np.asarray(dY, dtype=np.float64), np.asarray(X, dtype=np.float64)
    a_max = np.abs(dY).max() if a_max is None else a_max
    b_max = np.abs(X).max() if b_max is None else b_max
    Cout, Cin = dY.shape[2], X.shape[2]
    ref, bound = np.zeros((nsplit, Cout, batch, Cin)), np.zeros((nsplit, Cout, batch, Cin))
    for s in range(nsplit):
        r0, r1 = s * cps * BK, min(M, (s + 1) * cps * BK)
        for z in range(batch):
            A, B = dY[z, r0:r1].T, X[z, r0:r1]
            ref[s, :, z] = A @ B
            bound[s, :, z] = SB.gemm_bound(A, B, a_max, b_max) if arith == "h" else A_REL * EPS * (np.abs(A) @ np.abs(B))
    return ref, bound


def excess(got, ref, bound):
    return SB.excess(np.asarray(got, dtype=np.float64), ref, bound)


# ---- the kernels' order in numpy fp32 -------------------------------------------------------------------------------------------------
def _read(buf, off, C, ok):
    """rows of C floats at float offsets `off` of a flat buffer (reads past its end give NaN), zero where not ok"""
    buf = np.concatenate([np.asarray(buf, dtype=F32), F32([np.nan])])
    idx = np.minimum(off[..., None] + np.arange(C), len(buf) - 1)
    return np.where(ok[..., None], buf[idx], F32(0))


def _pieces(v, arith, e=0, once=False):
    with np.errstate(invalid="ignore", over="ignore"):
        if arith == "six":
            p = split3(v)[:3]
            if once:
                p = (bf16_rne(v), np.zeros_like(v), np.zeros_like(v))
        elif arith == "h":
            p = SB.split2(v, e)
        elif arith == "bf16op":
            p = (bf16_rne(v),)
        else:
            p = (v,)
    return [q.astype(np.float64) for q in p]


ORDER = {"six": [(2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0)], "h": [(1, 0), (0, 1), (0, 0)], "bf16op": [(0, 0)], "fp32": [(0, 0)]}


def emulate(dy, lddy, x, ldx, g, plan, choice, arith, g_obj=None, x_obj=None, prev=None, accumulate=0, reduce=True, fault=None):
    """dy / x: flat float32 buffers (pitches lddy / ldx), g: Geo, plan: (ctiles, nsplit, cps, last), choice: kernel_choice(...).
    Pixels in chunks of 32 and k blocks of 16 (2 for the fp32 matrix instruction); the products of a k block exact in float64, added to
    an fp32 accumulator, the piece products in the kernels' order; one accumulator per slab; the split-fp16 slab scaled back by
    2^-(e_dy + e_x); the slabs added in order onto 0 or the previous dw.  -> dw [Cout][R][S][Cin] float32 (reduce = False: the slabs
    [nsplit][Cout][R S][Cin], the batched entry points' output)"""
    assert fault is None or fault in FAULTS
    assert arith in ARITHS
    _, nsplit, cps, _ = plan
    taps, M = g.R * g.S, g.N * g.Hout * g.Wout
    nchunks = cdiv(M, BK)
    if fault == "pitch_ignored":
        lddy, ldx = g.Cout, g.Cin
    # index arithmetic of row_offsets / load_chunk for every pixel of every chunk
    m = np.arange(nchunks * BK)
    mv = np.ones_like(m, dtype=bool) if fault == "unmasked_rows" else m < M
    mm = np.where(mv, m, 0)
    t = mm // g.Wout
    wo, n = mm - t * g.Wout, t // g.Hout
    ho = t - n * g.Hout
    tap = np.arange(taps)
    r, s = tap // g.S, tap - (tap // g.S) * g.S
    if fault == "swap_rs":
        r, s = s, r
    step = g.mul if fault == "stride_as_dil" else g.step
    vh, vw = ho[None] * g.mul + g.off + r[:, None] * step, wo[None] * g.mul + g.off + s[:, None] * step       # [taps][pixels]
    okh, okw = (vh >= 0) & (vh < g.Hin), (vw >= 0) & (vw < g.Win)
    xrow = n[None] * g.Hin * g.Win + np.where(okh, vh, 0) * g.Win + np.where(okw, vw, 0)
    A = _read(dy, tap[:, None] * g.zdy + mm[None] * lddy, g.Cout, np.broadcast_to(mv, (taps, len(m))))        # [taps][pixels][Cout]
    B = _read(x, tap[:, None] * g.zx + xrow * ldx, g.Cin, mv[None] & okh & okw)                                # [taps][pixels][Cin]
    e_dy = e_x = 0
    if arith == "h":
        e_dy = SB.split2_exp(amax_value(g_obj, fault == "amax_shard0"))
        e_x = SB.split2_exp(amax_value(x_obj, fault == "amax_shard0"))
    pa, pb = _pieces(A, arith, e_dy, fault == "pass_bf16_once"), _pieces(B, arith, e_x)
    order = list(ORDER[arith])
    if fault == "drop_piece":
        del order[0]
    kb = 2 if arith == "fp32" else 16
    slabs = np.zeros((nsplit, g.Cout, taps, g.Cin), dtype=F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for sl in range(nsplit):
            c0, c1 = sl * cps, min(nchunks, (sl + 1) * cps)
            if fault == "skip_odd_tail" and (c1 - c0) % 2:
                c1 -= 1
            acc = np.zeros((taps, g.Cout, g.Cin), dtype=F32)
            for k0 in range(c0 * BK, c1 * BK, kb):
                for ia, ib in order:
                    acc = (acc.astype(np.float64) + np.matmul(pa[ia][:, k0:k0 + kb].transpose(0, 2, 1), pb[ib][:, k0:k0 + kb])).astype(F32)
            if arith == "h":
                acc = np.ldexp(acc.astype(np.float64), -(e_dy if fault == "scale_back_dy" else e_dy + e_x)).astype(F32)
            slabs[sl] = acc.transpose(1, 0, 2)
    flat = slabs.reshape(-1)
    wsz, rowlen = g.Cout * taps * g.Cin, taps * g.Cin
    if fault == "store_ci_past":        # the masked columns hold zeros; they land on the next tap's (or row's) first columns
        ci = np.arange(g.Cin, cdiv(g.Cin, choice.BN) * choice.BN)
        idx = (np.arange(nsplit)[:, None, None, None] * wsz + np.arange(g.Cout)[None, :, None, None] * rowlen
               + tap[None, None, :, None] * g.Cin + ci[None, None, None, :]).reshape(-1)
        flat[idx[idx < flat.size]] = 0
    if fault == "store_co_past":        # the masked rows hold zeros; they land on the next slab's first rows
        co = np.arange(g.Cout, cdiv(g.Cout, choice.BM) * choice.BM)
        idx = (np.arange(nsplit)[:, None, None] * wsz + co[None, :, None] * rowlen + np.arange(rowlen)[None, None, :]).reshape(-1)
        flat[idx[idx < flat.size]] = 0
    if not reduce:
        return slabs
    out = np.zeros((g.Cout, taps, g.Cin), dtype=F32)
    if accumulate and fault != "no_accumulate":
        out = np.asarray(prev, dtype=F32).reshape(out.shape).copy()
    with np.errstate(invalid="ignore", over="ignore"):
        for sl in range(nsplit - (1 if fault == "drop_last_slab" else 0)):
            out = (out + slabs[sl]).astype(F32)
    return out.reshape(g.Cout, g.R, g.S, g.Cin)


# ---- the table of edges ---------------------------------------------------------------------------------------------------------------
# name -> (N, H, W, k, stride, dil); EDGE: what the k_wgrad_tr plan at (Cin, Cout) = (128, 128) must be for the case to be the edge it
# is named for: (nsplit, cps, chunks in the last slab)
GEOMS = collections.OrderedDict([
    ("m25", (1, 5, 5, 1, 1, 1)), ("one_chunk", (1, 4, 8, 1, 1, 1)), ("nk2", (1, 8, 8, 1, 1, 1)), ("nk3", (1, 9, 9, 1, 1, 1)),
    ("nk5", (1, 13, 11, 1, 1, 1)), ("two_slabs", (1, 18, 21, 1, 1, 1)), ("ns7", (1, 35, 38, 1, 1, 1)), ("ns8", (1, 39, 39, 1, 1, 1)),
    ("ns9", (1, 40, 43, 1, 1, 1)), ("ns15", (1, 52, 55, 1, 1, 1)), ("ns17", (1, 57, 57, 1, 1, 1)), ("ns16_short", (1, 57, 60, 1, 1, 1)),
    ("g3x3", (2, 13, 11, 3, 1, 1)), ("dil12", (1, 7, 9, 3, 1, 12)), ("pw_s2", (2, 17, 15, 1, 2, 1)), ("g3x3_s2", (1, 21, 19, 3, 2, 1)),
])
EDGE = {"m25": (1, 1, 1), "one_chunk": (1, 1, 1), "nk2": (1, 2, 2), "nk3": (1, 3, 3), "nk5": (1, 5, 5), "two_slabs": (2, 6, 6),
        "ns7": (7, 6, 6), "ns8": (8, 6, 6), "ns9": (9, 6, 6), "ns15": (15, 6, 6), "ns17": (17, 6, 6), "ns16_short": (16, 7, 2),
        "g3x3": (1, 9, 9), "dil12": (1, 2, 2), "pw_s2": (1, 5, 5), "g3x3_s2": (1, 4, 4)}
# conv.hip's planner on the same geometries at one block tile per tap (any pair of at most 128 channels): its own slab counts
EDGE_CONV = {"ns7": (6, 7, 7), "ns8": (6, 8, 8), "ns9": (7, 8, 6), "ns15": (12, 8, 2), "ns17": (13, 8, 6), "ns16_short": (14, 8, 3),
             "two_slabs": (2, 6, 6), "g3x3": (2, 5, 4)}
WIDE = [(128, 128), (256, 128), (132, 128), (260, 132), (128, 260)]         # k_wgrad_tr's layers (Cin, Cout)
NARROW = [(64, 64), (64, 128), (128, 64), (68, 20), (32, 64)]                # conv.hip's four tile shapes
PAIRS = WIDE + NARROW
EVERY_PAIR = ("nk3", "ns9", "g3x3")
PITCHED = ("nk3", "ns9", "g3x3", "g3x3_s2")
BF16OP = [("nk3", (128, 128)), ("ns9", (68, 20)), ("g3x3", (64, 128)), ("g3x3_s2", (128, 64))]


def cases():
    """[(geometry name, (Cin, Cout))]: every geometry with (128, 128) and one other pair, every pair with the EVERY_PAIR geometries"""
    out = []
    for i, name in enumerate(GEOMS):
        out.append((name, (128, 128)))
        out.append((name, PAIRS[1 + i % (len(PAIRS) - 1)]))
    for p in PAIRS:
        for name in EVERY_PAIR:
            if (name, p) not in out:
                out.append((name, p))
    return out


def states(pair):
    """the switch states a channel pair runs under: (arith, split, tr, h); the narrow pairs are conv.hip's under either tr state"""
    if pair in WIDE:
        return [("h", 1, 1, 1), ("six", 1, 1, 0), ("six", 1, 0, 0), ("fp32", 0, 1, 0)]
    return [("six", 1, 1, 0), ("six", 1, 0, 0), ("fp32", 0, 0, 0)]


def case_operands(name, pair):
    """-> (Geo, pad, dy rows [M][Cout] six_decade_rows, x rows [N H W][Cin] relu_heavy_tail)"""
    N, H, W, k, stride, dil = GEOMS[name]
    Cin, Cout = pair
    g, pad = conv_geo(N, H, W, Cin, Cout, k, stride, dil)
    seed = 7 * list(GEOMS).index(name) + Cin + 3 * Cout
    return g, pad, rows("six_decade_rows", g.N * g.Hout * g.Wout, Cout, seed), rows("relu_heavy_tail", N * H * W, Cin, seed + 1)


def case_ref(name, pair, arith, dy, x, g_max=None, x_max=None, prev=None):
    N, H, W, k, stride, dil = GEOMS[name]
    g, pad = conv_geo(N, H, W, pair[0], pair[1], k, stride, dil)
    return dw_ref(nchw(dy, g.N, g.Hout, g.Wout), nchw(x, N, H, W), (k, k), stride, pad, dil, g_max, x_max, arith, prev)
