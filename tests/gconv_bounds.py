"""Shared by tests/test_gconv_cpu.py and tests/test_gpu_gconv.py: operands, float64 references with their bounds, the restated
launch plans, the shape table and a numpy float32 emulation of csrc/gconv.hip's addressing (with seven deliberate faults) for the
grouped convolution.

Oracle: torch.nn.functional.conv2d(groups=g) (and torch.nn.grad's input / weight gradients) in float64 on the CPU, on the
float32-rounded operands.  Bound of each output element, the derivation of tests/test_gpu_gconv.py:

    |got - ref| <= (n + 2) * 2^-24 * cond

cond: the same operation on absolute values (plus |bias| / |sink| where an epilogue adds one), n: the reduction length --
R*S*(Cin/groups) for y, R*S*(Cout/groups) for dx, N*Ho*Wo for dw.  This is the worst case of an fp32 sum of n products in any
order (n roundings of partial sums that never exceed cond) plus the bias / accumulate add: derived, not fitted.  The weight
gradient's slab partial sums fit it too: a term passes through at most (pixels per slab + slabs) <= n additions.  Where cond is 0
(taps that only ever meet padding) the bound is 0: the result must be exactly 0.

A case is (groups, cig, cog, R, S, H, W, stride, pad, dil, N) with cig = Cin/groups, cog = Cout/groups.  old_table() is what
tests/test_gpu_gconv.py ran before this module: WIDTHS x GEOMS (cig == cog, 3x3, pad = dil) and one 1x1.  new_cases() are the
paths of the kernels that table never reached; shape_list() is both."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from split_bounds import EPS, excess

NAMES = ("y", "dx", "dw")

# ---- the table --------------------------------------------------------------------------------------------------------------------
WIDTHS = [(32, 4), (32, 8), (8, 16), (4, 32), (2, 64), (3, 12)]                  # (groups, channels per group); last: generic width
GEOMS = [(13, 11, 1, 1), (9, 17, 2, 1), (13, 11, 1, 2), (9, 17, 1, 4), (12, 10, 2, 2)]      # (H, W, stride, dil)
N_IMG = 2
OLD_POINTWISE = (4, 32, 32, 1, 1, 9, 17, 2, 0, 1, N_IMG)

# (groups, cig, cog): cig != cog in both orders; 40 / 48 / 36: three column tiles on either side, the third one partial for 40 and 36;
# (3, 20, 52) and its mirror: a partial second and a partial fourth tile on either side, 2 against 4 tiles in the weight gradient
NEW_WIDTHS = [(4, 8, 16), (4, 16, 8), (2, 40, 48), (2, 48, 36), (3, 20, 52), (3, 52, 20)]
# (H, W, stride, dil), pad = dil: odd extents at stride 1, even extents at stride 2 with dilation 2, odd extents at stride 2
NEW_GEOMS = [(13, 11, 1, 1), (12, 10, 2, 2), (9, 17, 2, 1)]
# (2, 64, 60) as a 1x1: (H, W, stride)
POINTWISE_GEOMS = [(13, 11, 1), (9, 17, 2)]
KERNEL_CASES = [
    (8, 4, 12, 5, 5, 13, 11, 1, 2, 1, N_IMG),                   # 5x5
    (4, 12, 4, 5, 5, 12, 10, 2, 4, 2, N_IMG),                   # 5x5 at stride 2 and dilation 2
    (4, 8, 8, 1, 7, 9, 17, 1, 3, 1, N_IMG),                     # 1x7 with pad 3: Hout = Hin + 6
    (4, 8, 8, 7, 1, 9, 17, 1, 3, 1, N_IMG),                     # 7x1 with pad 3: Wout = Win + 6
    (2, 16, 16, 3, 5, 13, 11, 1, 1, 1, N_IMG),                  # 3x5
    (4, 8, 16, 2, 2, 12, 10, 2, 0, 1, N_IMG),                   # 2x2 at stride 2 and pad 0
]
# 11x11 on a 9x9 map, R*S = 121.  Dilation 4 with pad 20 (an output of 9x9): only the taps r, s in 3..7 ever land inside the map, the
# other 96 of the 121 meet padding alone (at dilation 1 and pad 5 every tap of an 11x11 kernel meets a 9x9 map somewhere)
BIG_KERNEL_CASE = (2, 4, 8, 11, 11, 9, 9, 1, 20, 4, N_IMG)
# pixel-count edges at (4, 8, 16) 3x3, stride 1, pad 1 (N*H*W pixels on either side): (N, H, W)
PIXEL_EDGES = [(5, 1, 1), (1, 1, 31), (2, 4, 4), (1, 3, 11), (1, 127, 1), (2, 8, 8), (1, 3, 43)]
WALK_CASE_IMAGES = (4, 8, 16, 3, 3, 1, 1, 1, 1, 1, 130)         # 130 images of 1x1: three slabs, a new image at every lane of the walk
WALK_CASE_NARROW = (4, 8, 16, 3, 3, 23, 3, 1, 1, 1, 3)          # Wout = 3: four slabs of 52 pixels, their edges inside image rows
SLAB_CAP_CASE = (2, 4, 4, 3, 3, 17, 128, 1, 1, 1, 16)           # M = 34816 > 64 * 512: 512 slabs of 68 pixels, their edges inside rows


def old_table():
    return [(g, cg, cg, 3, 3, H, W, stride, dil, dil, N_IMG) for g, cg in WIDTHS for H, W, stride, dil in GEOMS] + [OLD_POINTWISE]


def new_cases():
    out = [(g, ci, co, 3, 3, H, W, stride, dil, dil, N_IMG) for g, ci, co in NEW_WIDTHS for H, W, stride, dil in NEW_GEOMS]
    out += [(2, 64, 60, 1, 1, H, W, stride, 0, 1, N_IMG) for H, W, stride in POINTWISE_GEOMS]
    out += KERNEL_CASES + [BIG_KERNEL_CASE]
    out += [(4, 8, 16, 3, 3, H, W, 1, 1, 1, N) for N, H, W in PIXEL_EDGES]
    return out + [WALK_CASE_IMAGES, WALK_CASE_NARROW, SLAB_CAP_CASE]


def shape_list():
    """every case the GPU test runs the three entry points on"""
    return old_table() + new_cases()


def case_id(case):
    g, ci, co, R, S, H, W, stride, pad, dil, N = case
    return "g%d-%dto%d-%dx%d-n%d-%dx%d-s%d-p%d-d%d" % (g, ci, co, R, S, N, H, W, stride, pad, dil)


# ---- the plans of csrc/gconv.hip, restated -------------------------------------------------------------------------------------
def cdiv(a, b):
    return -(-a // b)


def out_size(h, k, stride, pad, dil):
    return (h + 2 * pad - dil * (k - 1) - 1) // stride + 1


def out_hw(case):
    g, ci, co, R, S, H, W, stride, pad, dil, N = case
    return out_size(H, R, stride, pad, dil), out_size(W, S, stride, pad, dil)


def pixels(case):
    """-> (pixels y is written on, pixels dx is written on)"""
    Ho, Wo = out_hw(case)
    return case[10] * Ho * Wo, case[10] * case[5] * case[6]


def conv_blocks(M, groups):
    """gconv_launch: -> (blocks of 128 pixels x one group, is the XCD remap on)"""
    n = cdiv(M, 128) * groups
    return n, n % 8 == 0


def col_tiles(c):
    """the JT of k_gconv's dispatch switch and the JT / CT of the weight gradient: 16-channel tiles of one group's channels"""
    return cdiv(c, 16)


def wgrad_plan(M, groups, cig, cog, RS):
    """gwgrad_plan: -> (pixels per slab, slabs NS, tiles = waves per slab, tap chunks ntc)"""
    ntc = 1 if RS in (1, 9) else RS
    tiles = groups * col_tiles(cog) * col_tiles(cig) * ntc
    ns = max(1, min(cdiv(8192, tiles), cdiv(M, 64), 512))
    rows = cdiv(cdiv(M, ns), 4) * 4
    return rows, cdiv(M, rows), tiles, ntc


def wgrad_family(RS):
    """the NT of k_gconv_wgrad<NT>: nine taps per wave for a 3x3, one otherwise"""
    return 9 if RS == 9 else 1


def workspace_bytes(case):
    g, ci, co, R, S = case[:5]
    return wgrad_plan(pixels(case)[0], g, ci, co, R * S)[1] * g * co * R * S * ci * 4


# ---- operands, references, bounds ------------------------------------------------------------------------------------------------
def operands(case, seed=0):
    """post-ReLU heavy-tailed x, weights N(0,1)/sqrt(R S cig), a gradient whose pixels span six decades (all float32, CPU); on the
    3x3 cases of old_table() these are the tensors of test_gpu_gconv._operands"""
    groups, cig, cog, R, S, H, W, stride, pad, dil, N = case
    g = torch.Generator().manual_seed(1000 * seed + 17 * groups + cig + (0 if cig == cog else 5 * cog))
    x = torch.relu(torch.randn(N, groups * cig, H, W, generator=g) - 0.25) ** 3
    w = torch.randn(groups * cog, cig, R, S, generator=g) / math.sqrt(R * S * cig)
    Ho, Wo = out_hw(case)
    gy = torch.randn(N, groups * cog, Ho, Wo, generator=g) * 1e-4 * 10.0 ** (-6 * torch.rand(N, 1, Ho, Wo, generator=g))
    return x, w, gy


def refs(case, x, w, gy, bias=None, sink=None):
    """float64 {name: (ref, bound)} of y, dx, dw"""
    groups, cig, cog, R, S, H, W, stride, pad, dil, N = case
    xd, wd, gd = x.double(), w.double(), gy.double()
    kw = dict(stride=stride, padding=pad, dilation=dil, groups=groups)

    def three(a, b, c):
        return (F.conv2d(a, b, **kw), torch.nn.grad.conv2d_input(tuple(x.shape), b, c, **kw),
                torch.nn.grad.conv2d_weight(a, tuple(w.shape), c, **kw))
    ref, cond = list(three(xd, wd, gd)), list(three(xd.abs(), wd.abs(), gd.abs()))
    if bias is not None:
        ref[0] = ref[0] + bias.double().view(1, -1, 1, 1)
        cond[0] = cond[0] + bias.double().abs().view(1, -1, 1, 1)
    if sink is not None:
        ref[2] = ref[2] + sink.double()
        cond[2] = cond[2] + sink.double().abs()
    ns = (R * S * cig, R * S * cog, gy.shape[0] * gy.shape[2] * gy.shape[3])
    return {name: (r, (n + 2) * EPS * c) for name, r, c, n in zip(NAMES, ref, cond, ns)}


def worst(got, ref_bounds, names=NAMES):
    """{name: largest |got - ref| / bound} (a bound of 0 asks for an exact 0)"""
    out = {}
    for name in names:
        ref, bound = ref_bounds[name]
        assert tuple(got[name].shape) == tuple(ref.shape), name
        out[name] = excess(got[name], ref, bound)
    return out


# ---- the kernels' addressing in numpy float32 ------------------------------------------------------------------------------------
FAULTS = {                  # name -> the outputs it can reach
    "dg_block_rows": ("dx",),               # the data gradient's group offset counts cig rows per group where cog are due
    "dg_role_stride": ("dx",),              # the role swap strides by RS * cog where RS * cig is due
    "tap_decode_R": ("y", "dx", "dw"),      # r = tap // R where tap // S is due
    "third_tile": ("y", "dx"),              # the dispatch switch has no case 3: channels 32..47 of a group are left 0 unless cd > 48
    "tap_chunk": ("dw",),                   # with ntc > 1 every wave takes and writes tap 0
    "ct_jt": ("dw",),                       # the weight gradient's tile decode uses JT where CT is due
    "row_wrap": ("dw",),                    # the pixel walk wraps at most one image row per step (an `if` for the `while`)
}
F32 = np.float32


def _rows(t):
    """(N, C, H, W) tensor -> float32 rows [N*H*W][C], the kernels' layout"""
    return np.ascontiguousarray(t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).numpy().astype(F32))


def _take(flat, idx):
    """flat[idx]; an index outside the array (a faulty emulation only) reads the nearest end instead of other memory"""
    return flat[np.clip(idx, 0, flat.size - 1)]


def _emulate_conv(src, wflat, case, dg, fault):
    """k_gconv<JT, DG>: rows [M][groups * cd] from the rows of the gathered side; all groups and all pixels at once, the reduction
    unit by unit (a unit: one tap, 4 consecutive channels of the gathered side)"""
    groups, cig, cog, R, S, H, W, stride, pad, dil, N = case
    Ho, Wo = out_hw(case)
    RS = R * S
    if dg:
        Hs, Ws, Hd, Wd, cs, cd = Ho, Wo, H, W, cog, cig
    else:
        Hs, Ws, Hd, Wd, cs, cd = H, W, Ho, Wo, cig, cog
    M, cu, sh = N * Hd * Wd, cs // 4, stride - 1
    P = np.arange(M)
    n, rem = P // (Hd * Wd), P % (Hd * Wd)
    hd, wd = rem // Wd, rem % Wd
    nb = n * Hs * Ws
    bh, bw = (hd + pad, wd + pad) if dg else (hd * stride - pad, wd * stride - pad)
    JT = col_tiles(cd)
    if fault == "third_tile" and JT == 3:
        JT = 2
    oc = np.arange(min(cd, 16 * JT))                                            # the columns the dispatched kernel owns
    g = np.arange(groups)
    block_rows = cd if (dg and fault == "dg_block_rows") else (cs if dg else cd)
    wg = g * block_rows * RS * cig                                              # this group's [cog][RS][cig] block
    src3 = src.reshape(-1, groups, cs)
    acc = np.zeros((M, groups, cd), F32)
    m = np.arange(4)
    for u in range(RS * cu):
        tap, cc = u // cu, u % cu
        r = tap // (R if fault == "tap_decode_R" else S)
        s = tap - r * S
        if dg:
            hh, ww = bh - r * dil, bw - s * dil
            ok = (hh >= 0) & (ww >= 0) & (((hh | ww) & sh) == 0)
            hi, wi = hh >> sh, ww >> sh
            ok &= (hi < Hs) & (wi < Ws)
        else:
            hi, wi = bh + r * dil, bw + s * dil
            ok = (hi >= 0) & (hi < Hs) & (wi >= 0) & (wi < Ws)
        row = np.where(ok, nb + hi * Ws + wi, 0)
        a = src3[row, :, 4 * cc:4 * cc + 4] * ok[:, None, None].astype(F32)     # [M][groups][4]
        if dg:      # w[out = 4cc + m][tap][in = oc]: the forward's weight with the channel roles swapped
            st = RS * (cog if fault == "dg_role_stride" else cig)
            q = wg[:, None, None] + (4 * cc * RS + tap) * cig + oc[None, :, None] + m[None, None, :] * st
        else:       # w[out = oc][tap][in = 4cc .. 4cc + 3]
            q = wg[:, None, None] + oc[None, :, None] * RS * cig + 4 * u + m[None, None, :]
        b = _take(wflat, q)                                                     # [groups][columns][4]
        acc[:, :, :oc.size] += np.einsum("pgm,gom->pgo", a, b)
    return acc.reshape(M, groups * cd)


def _walk(M, rows, NS, Ho, Wo, fault):
    """the pixel walk of k_gconv_wgrad for every slab and k-lane: -> (n, ho, wo, valid), each [NS][rows], decoded once per lane and
    advanced by 4 pixels per step without divisions"""
    steps = rows // 4
    s0 = np.arange(NS)[:, None] * rows
    s1 = np.minimum(s0 + rows, M)
    Pl = s0 + np.arange(4)[None, :]                                             # [NS][4 k-lanes]
    n, rem = Pl // (Ho * Wo), Pl % (Ho * Wo)
    ho, wo = rem // Wo, rem % Wo
    out = [np.zeros((NS, rows), np.int64) for _ in range(3)]
    valid = np.zeros((NS, rows), bool)
    for t in range(steps):
        sl = slice(4 * t, 4 * t + 4)
        out[0][:, sl], out[1][:, sl], out[2][:, sl] = n, ho, wo
        valid[:, sl] = (Pl + 4 * t) < s1
        wo = wo + 4
        for _ in range(1 if fault == "row_wrap" else cdiv(4, Wo) + 1):
            over = wo >= Wo
            wo = np.where(over, wo - Wo, wo)
            ho = ho + over
            up = ho >= Ho
            ho = np.where(up, 0, ho)
            n = n + up
    return out[0], out[1], out[2], valid


def _emulate_wgrad(xr, gr, case, fault):
    """k_gconv_wgrad<NT> + k_gconv_wgrad_finish: every wave's (slab, tap chunk, ct, jt, group) decoded as the kernel decodes it, its
    16 x 16 tile of per-slab sums written to the workspace, the slabs added in slab order -> [Cout][RS][cig]"""
    groups, cig, cog, R, S, H, W, stride, pad, dil, N = case
    Ho, Wo = out_hw(case)
    RS, M, Cout = R * S, N * Ho * Wo, groups * cog
    rows, NS, tiles, ntc = wgrad_plan(M, groups, cig, cog, RS)
    NT = wgrad_family(RS)
    JT, CT = col_tiles(cog), col_tiles(cig)
    n, ho, wo, valid = _walk(M, rows, NS, Ho, Wo, fault)
    valid &= n < N
    n = np.minimum(n, N - 1)
    Pw = np.where(valid, (n * Ho + ho) * Wo + wo, 0)
    a = gr[np.minimum(Pw, M - 1)] * valid[..., None].astype(F32)               # dy at the walk's pixels [NS][rows][Cout]
    a = a.reshape(NS, rows, groups, cog)
    full = np.zeros((NS, groups, cog, RS, cig), F32)                            # what a wave that owns (slab, tile, tap) sums up
    for tap in range(RS):
        r = tap // (R if fault == "tap_decode_R" else S)
        s = tap - r * S
        hi, wi = ho * stride + r * dil - pad, wo * stride + s * dil - pad
        ok = valid & (hi >= 0) & (hi < H) & (wi >= 0) & (wi < W)
        b = xr[np.where(ok, (n * H + hi) * W + wi, 0)] * ok[..., None].astype(F32)
        full[:, :, :, tap, :] = np.einsum("spgo,spgi->sgoi", a, b.reshape(NS, rows, groups, cig))
    part = np.zeros((NS, groups, cog, RS, cig), F32)
    for wid in range(tiles * NS):
        slab, rest = wid // tiles, wid % tiles
        tc, rest = rest % ntc, rest // ntc
        if fault == "ct_jt":
            ct, rest = rest % JT, rest // JT
        else:
            ct, rest = rest % CT, rest // CT
        jt, g = rest % JT, rest // JT
        tap0 = 0 if (fault == "tap_chunk" and ntc > 1) else tc * NT
        if g >= groups:                     # (a faulty decode only: the kernel would be outside the tensors here)
            continue
        o, i = slice(jt * 16, min(jt * 16 + 16, cog)), slice(ct * 16, min(ct * 16 + 16, cig))
        part[slab, g, o, tap0:tap0 + NT, i] = full[slab, g, o, tap0:tap0 + NT, i]
    dw = part[0].copy()
    for k in range(1, NS):                  # fixed order: slab 0, 1, ...
        dw = dw + part[k]
    return dw.reshape(Cout, RS, cig)


def emulate(case, x, w, gy, fault=None, names=NAMES):
    """y, dx, dw as csrc/gconv.hip addresses and sums them, in float32 (held to the bound, not to the kernels' bits).  Restated: the
    group's weight block offset, the unit and tap decode, the data gradient's role swap, the column-tile dispatch, the weight gradient's
    wave decode, tap chunks, pixel walk and slabs added in slab order.  fault: None or a key of FAULTS, one one-line mistake each."""
    assert fault is None or fault in FAULTS
    groups, cig, cog, R, S, H, W, stride, pad, dil, N = case
    Ho, Wo = out_hw(case)
    xr, gr = _rows(x), _rows(gy)
    wflat = np.ascontiguousarray(w.permute(0, 2, 3, 1).numpy().astype(F32)).reshape(-1)         # [Cout][R][S][cig]
    out = {}
    if "y" in names:
        y = _emulate_conv(xr, wflat, case, False, fault)
        out["y"] = torch.from_numpy(y.reshape(N, Ho, Wo, groups * cog)).permute(0, 3, 1, 2)
    if "dx" in names:
        dx = _emulate_conv(gr, wflat, case, True, fault)
        out["dx"] = torch.from_numpy(dx.reshape(N, H, W, groups * cig)).permute(0, 3, 1, 2)
    if "dw" in names:
        dw = _emulate_wgrad(xr, gr, case, fault)
        out["dw"] = torch.from_numpy(dw.reshape(groups * cog, R, S, cig)).permute(0, 3, 1, 2)
    return out
