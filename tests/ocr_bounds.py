"""Float64 references, numpy fp32 emulations, shape tables and error bounds of the object-contextual kernels in
u2pl_amd/csrc/ocr.hip (u2pl_region_pool_{fwd,bwd}_f32, u2pl_region_attn_{fwd,bwd}_f32), shared by tests/test_ocr_cpu.py and
tests/test_gpu_ocr.py.  Not a conftest: imported by name, like psp_bounds.

Arrays are rows: s, m, ds, w [N, HW, K]; x, add, dx [N, HW, C]; q, g_y, y, dq [N, HW, D]; f, g_f [N, K, C]; kk, v, dk, dv [N, K, D].
The backward references take the forward's saved outputs (m and f, w) as the inputs they are for the kernels: the fp32 values
handed to the kernel are the values the float64 formula is evaluated on.

Every element is held to  |got - ref64| <= EPS min(derived, CAL_MARGIN measured (1 + arg)) unit + floor  (EPS = 2^-24, one unit
per fp32 rounding; CAL_MARGIN of contrast_bounds).

  units     f: sum_p m |x|;  m and w: the value itself;  dx: sum_k m |g_f| + |add|;  ds: scale m (sum_c |g_f||x| + sum_c |g_f||f|);
            y: sum_k w |v|;  dv: sum_p w |g_y|;  with A_k = sum_d |g_y||v_k| and a = scale w_k (A_k + sum_j w_j A_j):
            dq: sum_k a |kk_k|, dk: sum_p a |q_p|.
  arg       the rounding of an exponent's argument, in units of EPS, is a RELATIVE error of the exponential and grows with the
            argument's range.  Region pool: t = scale s (error |t|), its column maximum M (|M|), t - M (|t - M|): arg = |t| + |M| +
            |t - M|.  Attention: t = scale dot (error |t| + dot_count scale sum |q||kk| = a_k), mx = max_k t (max_k a_k), t - mx:
            arg = a_k + max_k a_k + |t - mx|.  Outputs that sum over weights (f, y) take the largest arg of their weights.
  derived   roundings read off the straight-line code of ocr.hip; expf counts as 2.
            wave sum 6.  dot_count(C) = 4 (the product and three fma of a float4) + 6 + ceil(C / 256) (adds of the pass sums).
            col_count(HW, K) (Z of the pixel softmax): R = 256 / K rows, a slab of L = min(HW, 256) pixels: ceil(L / R) - 1 adds
            per row, min(R, L) - 1 row folds, ceil(HW / 256) - 1 slab adds.
            wsum_count(HW) (pixels -> regions): min(HW, 64) fma of a wave, <= 3 wave adds, ceil(HW / 256) - 1 slab adds.
            m:  e = expf(t - M): 2 + arg;  Z: sum_p m (2 + arg) + col_count;  one division:  (2 + arg) + sum_p m (2 + arg) +
                col_count + 1.           f: wsum_count + max_p (m's count).
            dx: K fma + 1 (add).         ds: max(dot_count, 4 ceil(C / 256) + 6 (c: one fma chain per lane, one wave sum)) + 3
                (the subtraction, scale m, the product).
            w:  e: 2 + arg; Z: sum_k w (2 + arg) + 3 + 6; one division.        y: K fma + max_k (w's count).
            e = (scale w)(dw - sd): dot_count (dw) + dot_count + 4 + 6 (sd: the lanes' fma chains, a wave sum) + 3 = E.
            dq: E + K.   dk: E + wsum_count.   dv: wsum_count.
  floor     a result below 2^-126 may be flushed to zero by expf or by a product (values there carry less than 24 bits in any
            case): every weight is allowed an absolute error of 2^-126 (m, w, and the m or w a backward is handed), which every
            output sees multiplied by the magnitude of what the weight multiplies (floor_* below).
  measured  what torch's own fp32 CPU arithmetic of the plain formulas reaches against float64 over OCR_HW x CAL_K at CAL_N,
            CAL_C, every family, in units of EPS (1 + arg) unit -- never a HIP kernel (python -m pytest tests/test_ocr_cpu.py -s
            -k ceilings; the emulation of the kernels' order in brackets):
                m   3.67 [1.64]    f   3.32 [1.27]    dx  3.92 [3.92]    ds  3.18 [2.08]
                w   0.23 [0.14]    y   0.12 [0.12]    dq  1.33 [1.14]    dk  1.50 [1.20]    dv  3.94 [3.77]
            (w and y are small numbers because they are in units of 1 + arg, and the attention's arg carries dot_count + 1
            roundings of scale sum |q||kk|, which is well above 1 on these tables.)

The emulations restate the kernels' order in numpy fp32 (fma as one rounding of the float64 product-sum; the pairing inside a
wave sum is a plain six-round tree: the count is the kernel's, the partners are not)."""
import numpy as np
import torch

from contrast_bounds import CAL_MARGIN
from glue_bounds import SENTINEL_BITS, bits_equal, rel_excess  # noqa: F401
from split_bounds import EPS

f32, f64 = np.float32, np.float64

# csrc/ocr.hip
SLAB = 256                      # OCR_SLAB: pixels of one slab
WAVE_PX = 64                    # OCR_WAVE_PX: pixels one wave of a weighted-sum block adds up
KT = 16                         # OCR_KT: regions of one weighted-sum work item
KCHUNK = 64                     # OCR_KCHUNK: regions per lane register of the per-pixel kernels
PX = 4                          # OCR_PX: pixels of one wave of the per-pixel kernels
PASS = 256                      # OCR_PASS: channels of one pass of a wave
GRID_CAP = 1024                 # OCR_MAX_BLOCKS
MAX_K = 255

OCR_N = (1, 3)
OCR_HW = ((1, 1), (2, 3), (7, 10), (33, 35), (1, SLAB + 1))                   # the last: the first size past one pixel slab
OCR_K = (1, 2, 19, 33, 255, KT - 1, KT, KT + 1, KCHUNK - 1, KCHUNK, KCHUNK + 1)
OCR_C = (4, 20, 64, 260)                                                    # 260: one float4 past a wave's pass
# 3 * 342 slabs > 1024 (column kernels, and weighted-sum items at one channel and one region chunk); 3 * 21825 pixel groups > 4 * 1024
GRID_CASE = dict(N=3, HW=(1, 342 * SLAB - 255), K=2, C=4)
# the two kernels that walk region rows, not pixels: k_region_wsum_reduce takes N K C / 4 float4 items in blocks of 256 threads
# (3 * 255 * 344 = 263160 > 256 * 1024), k_region_rowdot one wave per region row, four per block (17 * 255 = 4335 > 4 * 1024)
REDUCE_GRID_CASE = dict(N=3, HW=(1, 2), K=255, C=1376)
ROWDOT_GRID_CASE = dict(N=17, HW=(1, 1), K=255, C=4)
FAMILIES = ("normal", "big", "const")       # logits N(0, 2) / +-100 / class 0 constant
CAL_N, CAL_C, CAL_K = 3, 20, (1, 2, 19, 33)

# ---- calibrated ceilings: torch's own fp32 arithmetic against float64 (never the HIP kernels), rounded up by a few per cent
CAL = dict(m=3.8, f=3.45, dx=4.1, ds=3.3, w=0.24, y=0.13, dq=1.4, dk=1.55, dv=4.1)
TINY = 2.0 ** -126


def hw_of(HW):
    return HW[0] * HW[1]


def pool_scale(N):
    return 1.0 if N == 1 else 0.7


def attn_scale(D):
    return float(D) ** -0.5


def pool_case(N, HW, K, C, family="normal", seed=0):
    """-> s [N, HW, K], x [N, HW, C], g_f [N, K, C], add [N, HW, C]  (float32)"""
    rng = np.random.default_rng([seed, 41, N, HW, K, C, FAMILIES.index(family)])
    s = rng.standard_normal((N, HW, K), dtype=f32) * f32(2)
    if family == "big":
        s = (np.where(rng.random((N, HW, K)) < 0.5, f32(-100), f32(100)) + s).astype(f32)
    if family == "const":
        s[:, :, 0] = f32(1.25)
    x = rng.standard_normal((N, HW, C), dtype=f32) + f32(0.5)
    g = rng.standard_normal((N, K, C), dtype=f32)
    add = rng.standard_normal((N, HW, C), dtype=f32)
    return s, x, g, add


def attn_case(N, HW, K, D, family="normal", seed=0):
    """-> q [N, HW, D], kk [N, K, D], v [N, K, D], g_y [N, HW, D]; big: logits scale q . kk of about +-100"""
    rng = np.random.default_rng([seed, 43, N, HW, K, D, FAMILIES.index(family)])
    q = rng.standard_normal((N, HW, D), dtype=f32)
    kk = rng.standard_normal((N, K, D), dtype=f32)
    if family == "big":
        q = (q * f32(100)).astype(f32)
    if family == "const":
        kk[:, :, :] = kk[:, :1, :]           # every region has the same key: the weights are 1 / K
    v = rng.standard_normal((N, K, D), dtype=f32) + f32(0.5)
    gy = rng.standard_normal((N, HW, D), dtype=f32)
    return q, kk, v, gy


# =================================================================== float64 references ========================================
def d64(*a):
    return [np.asarray(t, dtype=f64) for t in a]


def cdiv(a, b):
    return -(-a // b)


def softmax64(t, axis):
    e = np.exp(t - t.max(axis=axis, keepdims=True))
    return e / e.sum(axis=axis, keepdims=True)


def T_(a):
    return np.swapaxes(a, 1, 2)


def pool_fwd64(s, x, scale):
    """-> dict(m, f, unit_f, arg [N, HW, K])"""
    s, x = d64(s, x)
    t = f64(f32(scale)) * s
    M = t.max(axis=1, keepdims=True)
    m = softmax64(t, 1)
    return dict(m=m, f=T_(m) @ x, unit_f=T_(m) @ np.abs(x), arg=np.abs(t) + np.abs(M) + np.abs(t - M), sumx=np.abs(x).sum(1))


def pool_bwd64(g, m, x, f, add, scale):
    """m, f: the forward's outputs as handed to the kernel; g or add may be None -> dict(dx, ds, unit_dx, unit_ds)"""
    m, x, f = d64(m, x, f)
    sc = f64(f32(scale))
    dx, udx, fdx = np.zeros(x.shape), np.zeros(x.shape), 0.0
    ds, uds, fds = np.zeros(m.shape), np.zeros(m.shape), 0.0
    if g is not None:
        g = np.asarray(g, dtype=f64)
        dx, udx = m @ g, m @ np.abs(g)
        c, uc = (g * f).sum(2), (np.abs(g) * np.abs(f)).sum(2)
        ds = sc * m * (x @ T_(g) - c[:, None, :])
        mag = abs(sc) * (np.abs(x) @ T_(np.abs(g)) + uc[:, None, :])
        uds, fds, fdx = m * mag, TINY * (1.0 + mag), TINY * np.abs(g).sum(1)[:, None, :]
    if add is not None:
        dx, udx = dx + np.asarray(add, dtype=f64), udx + np.abs(np.asarray(add, dtype=f64))
    return dict(dx=dx, ds=ds, unit_dx=udx, unit_ds=uds, floor_dx=fdx, floor_ds=fds)


def attn_fwd64(q, kk, v, scale):
    q, kk, v = d64(q, kk, v)
    sc = f64(f32(scale))
    t = sc * (q @ T_(kk))
    a = abs(sc) * (np.abs(q) @ T_(np.abs(kk))) * (dot_count(q.shape[2]) + 1)
    mx = t.max(axis=2, keepdims=True)
    w = softmax64(t, 2)
    return dict(w=w, y=w @ v, unit_y=w @ np.abs(v), arg=a + a.max(axis=2, keepdims=True) + np.abs(t - mx), sumv=np.abs(v).sum(1))


def attn_bwd64(gy, w, q, kk, v, scale):
    """w: the forward's output as handed to the kernel -> dict(dq, dk, dv, unit_*)"""
    gy, w, q, kk, v = d64(gy, w, q, kk, v)
    sc = f64(f32(scale))
    dw, A = gy @ T_(v), np.abs(gy) @ T_(np.abs(v))
    e = sc * w * (dw - (w * dw).sum(2, keepdims=True))
    mag = abs(sc) * (A + (w * A).sum(2, keepdims=True))
    a = w * mag
    return dict(dq=e @ kk, dk=T_(e) @ q, dv=T_(w) @ gy, unit_dq=a @ np.abs(kk), unit_dk=T_(a) @ np.abs(q), unit_dv=T_(w) @ np.abs(gy),
                floor_dq=TINY * ((1.0 + mag) @ np.abs(kk)), floor_dk=TINY * (T_(1.0 + mag) @ np.abs(q)),
                floor_dv=TINY * np.abs(gy).sum(1)[:, None, :])


# =================================================================== counts and bounds ==========================================
def dot_count(C):
    return 4 + 6 + cdiv(C, PASS)


def col_count(HW, K):
    R, L = SLAB // K, min(HW, SLAB)
    return (cdiv(L, R) - 1) + (min(R, L) - 1) + (cdiv(HW, SLAB) - 1)


def wsum_count(HW):
    return min(HW, WAVE_PX) + min(3, cdiv(min(HW, SLAB), WAVE_PX) - 1) + (cdiv(HW, SLAB) - 1)


def _b(derived, cal, arg=0.0):
    return np.minimum(derived, CAL_MARGIN * cal * (1.0 + arg))


def pool_fwd_excess(got_m, got_f, s, x, scale):
    """-> (excess of m, excess of f)"""
    r = pool_fwd64(s, x, scale)
    HW, K = s.shape[1:]
    e = 2.0 + r["arg"]
    cm = e + (r["m"] * e).sum(1, keepdims=True) + col_count(HW, K) + 1
    em = rel_excess(got_m, r["m"], EPS * _b(cm, CAL["m"], r["arg"]) * r["m"] + TINY)
    argf = r["arg"].max(1)[:, :, None]
    cf = wsum_count(HW) + cm.max(1)[:, :, None]
    ef = rel_excess(got_f, r["f"], EPS * _b(cf, CAL["f"], argf) * r["unit_f"] + TINY * r["sumx"][:, None, :])
    return em, ef


def pool_bwd_excess(got_dx, got_ds, g, m, x, f, add, scale):
    """got_dx or got_ds may be None (that output was not asked for)"""
    r = pool_bwd64(g, m, x, f, add, scale)
    K, C = m.shape[2], x.shape[2]
    cdx = (K if g is not None else 0) + (1 if add is not None else 0)
    cds = max(dot_count(C), 4 * cdiv(C, PASS) + 6) + 3
    edx = 0.0 if got_dx is None else rel_excess(got_dx, r["dx"], EPS * _b(cdx, CAL["dx"]) * r["unit_dx"] + r["floor_dx"])
    eds = 0.0 if got_ds is None else rel_excess(got_ds, r["ds"], EPS * _b(cds, CAL["ds"]) * r["unit_ds"] + r["floor_ds"])
    return edx, eds


def attn_fwd_excess(got_w, got_y, q, kk, v, scale):
    r = attn_fwd64(q, kk, v, scale)
    K = kk.shape[1]
    e = 2.0 + r["arg"]
    cw = e + (r["w"] * e).sum(2, keepdims=True) + 9 + 1
    ew = rel_excess(got_w, r["w"], EPS * _b(cw, CAL["w"], r["arg"]) * r["w"] + TINY)
    cy = K + cw.max(2, keepdims=True)
    ey = rel_excess(got_y, r["y"], EPS * _b(cy, CAL["y"], r["arg"].max(2, keepdims=True)) * r["unit_y"] + TINY * r["sumv"][:, None, :])
    return ew, ey


def attn_bwd_excess(got, gy, w, q, kk, v, scale):
    """got: dict with any of dq, dk, dv -> dict of excesses"""
    r = attn_bwd64(gy, w, q, kk, v, scale)
    HW, D = q.shape[1:]
    K = kk.shape[1]
    E = 2 * dot_count(D) + 13
    cnt = dict(dq=E + K, dk=E + wsum_count(HW), dv=wsum_count(HW))
    return {k: rel_excess(got[k], r[k], EPS * _b(cnt[k], CAL[k]) * r["unit_" + k] + r["floor_" + k]) for k in got}


# =================================================================== numpy fp32 emulations of the kernels' own order ============
def fma(a, b, c):
    return (np.asarray(a, dtype=f64) * np.asarray(b, dtype=f64) + np.asarray(c, dtype=f64)).astype(f32)


def wave_sum(v):
    """[..., 64] -> [...]: six pairwise rounds"""
    o = 32
    while o:
        v = (v[..., :o] + v[..., o:2 * o]).astype(f32)
        o //= 2
    return v[..., 0]


def emu_dot(rows, x):
    """rows [N, K, C], x [N, HW, C] -> [N, HW, K]: ocr_dots"""
    N, K, C = rows.shape
    Cp = cdiv(C, PASS) * PASS
    r = np.zeros((N, 1, K, Cp), dtype=f32)
    r[:, 0, :, :C] = rows
    xx = np.zeros((N, x.shape[1], 1, Cp), dtype=f32)
    xx[:, :, 0, :C] = x
    d = np.zeros((N, x.shape[1], K), dtype=f32)
    for c0 in range(0, Cp, PASS):
        a = r[..., c0:c0 + PASS].reshape(N, 1, K, 64, 4)
        b = xx[..., c0:c0 + PASS].reshape(N, -1, 1, 64, 4)
        p = (a[..., 0] * b[..., 0]).astype(f32)
        for j in (1, 2, 3):
            p = fma(a[..., j], b[..., j], p)
        d = (d + wave_sum(p)).astype(f32)
    return d


def emu_rowdot(g, f):
    """[N, K, C] x [N, K, C] -> [N, K]: k_region_rowdot"""
    N, K, C = g.shape
    Cp = cdiv(C, PASS) * PASS
    a, b = np.zeros((N, K, Cp), dtype=f32), np.zeros((N, K, Cp), dtype=f32)
    a[..., :C], b[..., :C] = g, f
    p = np.zeros((N, K, 64), dtype=f32)
    for c0 in range(0, Cp, PASS):
        aa, bb = a[..., c0:c0 + PASS].reshape(N, K, 64, 4), b[..., c0:c0 + PASS].reshape(N, K, 64, 4)
        for j in range(4):
            p = fma(aa[..., j], bb[..., j], p)
    return wave_sum(p)


def emu_mix(wt, rows, add=None):
    """wt [N, HW, K], rows [N, K, C] -> [N, HW, C]: ocr_mix"""
    acc = np.zeros((wt.shape[0], wt.shape[1], rows.shape[2]), dtype=f32)
    for k in range(rows.shape[1]):
        acc = fma(wt[:, :, k, None], rows[:, None, k, :], acc)
    return acc if add is None else (acc + add).astype(f32)


def emu_wsum(a, x):
    """a [N, HW, K], x [N, HW, C] -> [N, K, C]: k_region_wsum + k_region_wsum_reduce"""
    N, HW, K = a.shape
    out = None
    for p0 in range(0, HW, SLAB):
        slab = None
        for w0 in range(p0, min(HW, p0 + SLAB), WAVE_PX):
            acc = np.zeros((N, K, x.shape[2]), dtype=f32)
            for p in range(w0, min(HW, w0 + WAVE_PX)):
                acc = fma(a[:, p, :, None], x[:, p, None, :], acc)
            slab = acc if slab is None else (slab + acc).astype(f32)
        out = slab if out is None else (out + slab).astype(f32)
    return out


def emu_colsum(e):
    """e [N, HW, K] -> [N, K]: k_region_colsum's order (R = 256 / K rows per slab, row folds, slabs ascending)"""
    N, HW, K = e.shape
    R = SLAB // K
    out = None
    for p0 in range(0, HW, SLAB):
        blk = e[:, p0:p0 + SLAB]
        L = blk.shape[1]
        pad = np.zeros((N, cdiv(L, R) * R, K), dtype=f32)
        pad[:, :L] = blk
        pad = pad.reshape(N, -1, R, K)
        rows = np.zeros((N, R, K), dtype=f32)
        for j in range(pad.shape[1]):
            rows = (rows + pad[:, j]).astype(f32)
        z = rows[:, 0]
        for r in range(1, R):
            z = (z + rows[:, r]).astype(f32)
        out = z if out is None else (out + z).astype(f32)
    return out


FAULTS_POOL_FWD = ("no_max", "over_classes", "whole_batch")
FAULTS_POOL_BWD = ("no_c",)
FAULTS_ATTN_FWD = ("no_max", "no_scale")
FAULTS_ATTN_BWD = ("no_sd", "dk_no_scale")


def emu_pool_fwd(s, x, scale, fault=None):
    """u2pl_region_pool_fwd_f32 -> (m, f).  Faults: no_max (exponentials of the raw logits), over_classes (the softmax runs over
    the K classes of a pixel), whole_batch (maximum and sum over the pixels of every image together)"""
    N, HW, K = s.shape
    with np.errstate(over="ignore", invalid="ignore"):
        t = (f32(scale) * s).astype(f32)
        if fault == "over_classes":
            e = np.exp((t - t.max(2, keepdims=True)).astype(f32)).astype(f32)
            m = (e / e.sum(2, keepdims=True, dtype=f32)).astype(f32)
            return m, emu_wsum(m, x)
        if fault == "whole_batch":
            t = t.reshape(1, N * HW, K)
        M = np.zeros((t.shape[0], 1, K), dtype=f32) if fault == "no_max" else t.max(1, keepdims=True)
        e = np.exp((t - M).astype(f32)).astype(f32)
        m = (e / emu_colsum(e)[:, None, :]).astype(f32).reshape(N, HW, K)
    return m, emu_wsum(m, x)


def emu_pool_bwd(g, m, x, f, add, scale, fault=None):
    """u2pl_region_pool_bwd_f32 -> (dx, ds).  Fault: no_c (the - c[n, k] term dropped)"""
    if g is None:
        return (np.zeros(x.shape, dtype=f32) if add is None else add.copy()), np.zeros(m.shape, dtype=f32)
    d = emu_dot(g, x)
    if fault != "no_c":
        d = (d - emu_rowdot(g, f)[:, None, :]).astype(f32)
    ds = ((f32(scale) * m).astype(f32) * d).astype(f32)
    return emu_mix(m, g, add), ds


def emu_softmax_k(t, fault=None):
    """the attention's softmax over the regions: lane l holds the regions l, l + 64, ..."""
    K = t.shape[2]
    with np.errstate(over="ignore", invalid="ignore"):
        mx = np.zeros(t.shape[:2] + (1,), dtype=f32) if fault == "no_max" else t.max(2, keepdims=True)
        e = np.exp((t - mx).astype(f32)).astype(f32)
        lanes = np.zeros(t.shape[:2] + (4, 64), dtype=f32)
        lanes.reshape(t.shape[:2] + (256,))[..., :K] = e
        z = lanes[..., 0, :]
        for r in (1, 2, 3):
            z = (z + lanes[..., r, :]).astype(f32)
        return (e / wave_sum(z)[..., None]).astype(f32)


def emu_attn_fwd(q, kk, v, scale, fault=None):
    """u2pl_region_attn_fwd_f32 -> (w, y).  Faults: no_max, no_scale (the logits are the raw dot products)"""
    d = emu_dot(kk, q)
    t = d if fault == "no_scale" else (f32(scale) * d).astype(f32)
    w = emu_softmax_k(t, fault)
    return w, emu_mix(w, v)


def emu_attn_bwd(gy, w, q, kk, v, scale, fault=None):
    """u2pl_region_attn_bwd_f32 -> dict(dq, dk, dv).  Faults: no_sd (the - sum_k w dw term dropped), dk_no_scale"""
    N, HW, K = w.shape
    dw = emu_dot(v, gy)
    lw, ld = np.zeros((N, HW, 4, 64), dtype=f32), np.zeros((N, HW, 4, 64), dtype=f32)
    lw.reshape(N, HW, 256)[..., :K] = w
    ld.reshape(N, HW, 256)[..., :K] = dw
    sd = (lw[:, :, 0] * ld[:, :, 0]).astype(f32)
    for r in (1, 2, 3):
        sd = fma(lw[:, :, r], ld[:, :, r], sd)
    sd = wave_sum(sd)[..., None]
    diff = dw if fault == "no_sd" else (dw - sd).astype(f32)
    e = ((f32(scale) * w).astype(f32) * diff).astype(f32)
    ek = (w * diff).astype(f32) if fault == "dk_no_scale" else e
    return dict(dq=emu_mix(e, kk), dk=emu_wsum(ek, q), dv=emu_wsum(w, gy))


# =================================================================== torch's own fp32 arithmetic of the plain formulas ============
def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def torch_pool_fwd(s, x, scale):
    m = torch.softmax(T(s) * f32(scale), 1)
    return m.numpy(), (m.transpose(1, 2) @ T(x)).numpy()


def torch_pool_bwd(g, m, x, f, add, scale):
    g, m, x, f = T(g), T(m), T(x), T(f)
    dx = m @ g + T(add)
    ds = f32(scale) * m * (x @ g.transpose(1, 2) - (g * f).sum(2)[:, None, :])
    return dx.numpy(), ds.numpy()


def torch_attn_fwd(q, kk, v, scale):
    w = torch.softmax((T(q) @ T(kk).transpose(1, 2)) * f32(scale), 2)
    return w.numpy(), (w @ T(v)).numpy()


def torch_attn_bwd(gy, w, q, kk, v, scale):
    gy, w, q, kk, v = T(gy), T(w), T(q), T(kk), T(v)
    dw = gy @ v.transpose(1, 2)
    e = f32(scale) * w * (dw - (w * dw).sum(2, keepdim=True))
    return dict(dq=(e @ kk).numpy(), dk=(e.transpose(1, 2) @ q).numpy(), dv=(w.transpose(1, 2) @ gy).numpy())


def _ratio(got, ref, unit, arg=0.0, floor=0.0):
    return rel_excess(got, ref, EPS * (1.0 + arg) * np.asarray(unit, dtype=f64) + floor + 1e-300)


def measure(form="torch"):
    """-> {output: largest error in EPS (1 + arg) unit} over OCR_HW x CAL_K x FAMILIES at CAL_N, CAL_C"""
    worst = dict.fromkeys(CAL, 0.0)

    def up(k, v):
        worst[k] = max(worst[k], v)
    for HW in OCR_HW:
        for K in CAL_K:
            for fam in FAMILIES:
                N, C, hw = CAL_N, CAL_C, hw_of(HW)
                s, x, g, add = pool_case(N, hw, K, C, fam)
                sc = pool_scale(N)
                r = pool_fwd64(s, x, sc)
                m, f = torch_pool_fwd(s, x, sc) if form == "torch" else emu_pool_fwd(s, x, sc)
                up("m", _ratio(m, r["m"], r["m"], r["arg"], TINY))
                up("f", _ratio(f, r["f"], r["unit_f"], r["arg"].max(1)[:, :, None], TINY * r["sumx"][:, None, :]))
                m32, f32_ = r["m"].astype(f32), r["f"].astype(f32)
                b = pool_bwd64(g, m32, x, f32_, add, sc)
                dx, ds = torch_pool_bwd(g, m32, x, f32_, add, sc) if form == "torch" else emu_pool_bwd(g, m32, x, f32_, add, sc)
                up("dx", _ratio(dx, b["dx"], b["unit_dx"], 0.0, b["floor_dx"]))
                up("ds", _ratio(ds, b["ds"], b["unit_ds"], 0.0, b["floor_ds"]))
                q, kk, v, gy = attn_case(N, hw, K, C, fam)
                sc = attn_scale(C)
                r = attn_fwd64(q, kk, v, sc)
                w, y = torch_attn_fwd(q, kk, v, sc) if form == "torch" else emu_attn_fwd(q, kk, v, sc)
                up("w", _ratio(w, r["w"], r["w"], r["arg"], TINY))
                up("y", _ratio(y, r["y"], r["unit_y"], r["arg"].max(2, keepdims=True), TINY * r["sumv"][:, None, :]))
                w32 = r["w"].astype(f32)
                b = attn_bwd64(gy, w32, q, kk, v, sc)
                got = torch_attn_bwd(gy, w32, q, kk, v, sc) if form == "torch" else emu_attn_bwd(gy, w32, q, kk, v, sc)
                for k in ("dq", "dk", "dv"):
                    up(k, _ratio(got[k], b[k], b["unit_" + k], 0.0, b["floor_" + k]))
    return worst


# =================================================================== device buffers (GPU file) =================================
def sentinel():
    return np.array([SENTINEL_BITS], dtype=np.uint32).view(f32)[0]
