"""Float64 references, numpy fp32 emulations, shape tables and error bounds of the criss-cross attention kernels in
u2pl_amd/csrc/ccattn.hip (u2pl_cc_attn_{fwd,bwd}_f32), shared by tests/test_cc_cpu.py and tests/test_gpu_cc.py.  Not a conftest:
imported by name, like ocr_bounds.

Arrays are maps: q, k, dq, dk [N, H, W, D]; v, res, out, g, dv [N, H, W, C]; w [N, H, W, L], L = H + W - 1, in the header's slot
layout: for the pixel (y, x) slot j < W is (y, j) and slot W + i - (i > y) is (i, x), i != y.  gamma and scale are floats.
The backward references take the forward's saved w as the input it is for the kernel: the fp32 values handed to the kernel are
the values the float64 formula is evaluated on.

The float64 reference is torch's autograd of the DENSE masked attention (dense64: an [H W, H W] score matrix per image, masked to
the cross); plain() states the same formulas on the rows and columns (matrix products per image row and per image column) in a
dtype of choice: in float64 it is what the bounds are taken against (tests/test_cc_cpu.py holds it to dense64 in three score
families), in float32 it is "torch's own fp32 arithmetic of the plain formulas" that the ceilings are measured from.

Every element is held to  |got - ref64| <= EPS min(derived, CAL_MARGIN measured (1 + arg)) unit + floor  (EPS = 2^-24, one unit
per fp32 rounding; CAL_MARGIN of contrast_bounds).

  units     w: the value itself;  out: |gamma| sum_m w |v| + |res|;  dv: |gamma| sum_{p in X(m)} w[p, m] |g[p]|;
            with A[p, m] = sum_c |g[p]||v[m]| and a = |scale gamma| w (A + sum_j w_j A_j):  dq: sum_m a[p, m] |k[m]|,
            dk: sum_{p in X(m)} a[p, m] |q[p]|;  dgamma: sum_{n, p, m} w A.
  arg       the rounding of an exponent's argument, in units of EPS, is a RELATIVE error of the exponential (ocr_bounds, DESIGN
            3.16): u = scale dot (error |u| + dot_count |scale| sum |q||k| = a_m), mx = max_m u (max_m a_m), u - mx:
            arg = a_m + max_m a_m + |u - mx|.  out takes the largest arg of its weights.
  derived   roundings read off the straight-line code of ccattn.hip; expf counts as 2.
            dot_count(D) = D (one fma chain over the channels).  lane_count(L) = ceil(L / 64) - 1 adds of a lane's registers;
            wave sum 6.
            w:   e = expf(u - mx): 2 + arg;  Z: sum_m w (2 + arg) + lane_count + 6;  one division:
                 (2 + arg) + sum_m w (2 + arg) + lane_count + 6 + 1.
            out: L fma + 1 (the finish) + max_m (w's count).
            e = ((scale gamma) w)(t - s): t: dot_count(C); s: dot_count(C) + lane_count + 1 + 6; scale gamma, its product
                 with w, the subtraction, the product: 4.   E = 2 dot_count(C) + lane_count + 11.
            dq: E + L.   dk: E + L.   dv: L + 1 (gamma).
            dgamma: dot_count(C) + lane_count + 7 + sum_count(N H W), sum_count(P) = ceil(P / 1024) + 31 + 31.
  floor     a result below 2^-126 may be flushed to zero by expf or by a product: every weight (and e) is allowed an absolute
            error of 2^-126, which every output sees multiplied by the magnitude of what the weight multiplies (floor_*).
  measured  what torch's own fp32 CPU arithmetic of the plain formulas (plain(..., torch.float32)) reaches against float64 over
            CAL_HW x CAL_NDC x FAMILIES, in units of EPS (1 + arg) unit -- never a HIP kernel (python -m pytest
            tests/test_cc_cpu.py -s -k ceilings; the emulation of the kernels' order in brackets):
                w   0.42 [0.43]    out 0.58 [0.58]    dq  1.35 [1.54]    dk  2.14 [2.34]    dv  5.61 [5.61]    dgamma 1.71 [0.57]
            (w and out are in units of 1 + arg, and arg carries dot_count + 1 roundings of |scale| sum |q||k|: at D = 20 they are
            below 0.1; the figures above come from D = 4 with every key the same, where arg is small and the roundings of the
            sums over the cross are what is left.)

The emulations restate the kernels' order in numpy fp32 (fma as one rounding of the float64 product-sum; the pairing inside a
wave sum is a plain six-round tree: the count is the kernel's, the partners are not)."""
import numpy as np
import torch

from contrast_bounds import CAL_MARGIN
from glue_bounds import SENTINEL_BITS, bits_equal, rel_excess  # noqa: F401
from ocr_bounds import cdiv, fma, sentinel, wave_sum  # noqa: F401
from split_bounds import EPS

f32, f64 = np.float32, np.float64

# csrc/ccattn.hip
MAX_L = 512                     # CC_MAX_L
LCHUNK = 64                     # CC_LCHUNK: slots per lane register of the per-pixel kernels; members per k_cc_dots work item
LREGS = 8                       # CC_LREGS
PT = 8                          # CC_PT: consecutive pixels of a line taken by one wave of k_cc_dots / k_cc_mix
PASS = 256                      # CC_PASS: channels of one k_cc_mix work item
GRID_CAP = 1024                 # CC_MAX_BLOCKS (four waves a block)
SUM_THREADS = 1024              # CC_SUM_THREADS

# the maps of the GPU file: the smallest crosses, H != W both ways, the group edge (PT) along both lines, the lane edges of the
# per-pixel kernels (L = 63 / 64 / 65, ...) and of k_cc_dots (a line of 63 .. 65, 127 .. 129 members), the limit
CC_HW = ((1, 1), (1, 7), (7, 1), (2, 2), (3, 5), (5, 3), (9, 17),
         (32, 32), (32, 33), (33, 33),                                      # L = 63, 64, 65
         (2, 63), (2, 64), (65, 2),                                         # a line of 63, 64, 65 members
         (2, 126), (2, 127), (128, 2), (2, 129),                            # L = 127, 128, 129, 130; lines of 126 .. 129
         (2, 254), (255, 2), (2, 256),                                      # L = 255, 256, 257
         (2, MAX_L - 2), (2, MAX_L - 1), (MAX_L - 1, 2), (1, MAX_L), (MAX_L, 1))   # L = 511, 512
CC_NDC = ((1, 4, 4), (1, 260, 4), (3, 20, 64), (3, 64, 260))                # (N, D, C); 260: one float4 past a k_cc_mix pass
# every kernel takes a second trip of its grid-stride loop: 2100 * 16 pixels > 4096 waves; k_cc_dots / k_cc_mix row items
# 2100 * 2 lines * 1 group = 4200 > 4096, column items 2100 * 8 lines; and k_cc_sum walks 33600 > 32 * 1024 partials
GRID_CASE = dict(N=2100, HW=(2, 8), D=4, C=4)
FAMILIES = ("normal", "big", "const")       # scores N(0, 2) / +-100 / every key the same
CAL_NDC = ((3, 20, 20), (1, 4, 4))          # (1, 4, 4): short dots, a small arg: the roundings of the sums over the cross show
CAL_HW = ((1, 1), (1, 7), (7, 1), (2, 2), (3, 5), (5, 3), (9, 17), (33, 2), (2, 66))

# ---- calibrated ceilings: torch's own fp32 arithmetic against float64 (never the HIP kernels), rounded up by a few per cent
CAL = dict(w=0.44, out=0.6, dq=1.4, dk=2.2, dv=5.8, dgamma=1.8)
TINY = 2.0 ** -126
OUTS_BWD = ("dq", "dk", "dv", "dgamma")


def case_scale(D):
    """so that q . k of standard normal rows has the variance 2: the score family N(0, 2)"""
    return float(np.sqrt(2.0 / D))


def cc_case(N, HW, D, C, family="normal", seed=0):
    """-> q, k [N, H, W, D], v, res, g [N, H, W, C] (float32); big: scores scale q . k of about +-100"""
    H, W = HW
    rng = np.random.default_rng([seed, 47, N, H, W, D, C, FAMILIES.index(family)])
    q = rng.standard_normal((N, H, W, D), dtype=f32)
    k = rng.standard_normal((N, H, W, D), dtype=f32)
    if family == "big":
        q = (q * f32(100 / np.sqrt(2.0))).astype(f32)
    if family == "const":
        k[:] = k[:, :1, :1, :]                   # every pixel has the same key: the weights are 1 / L
    v = rng.standard_normal((N, H, W, C), dtype=f32) + f32(0.5)
    res = rng.standard_normal((N, H, W, C), dtype=f32)
    g = rng.standard_normal((N, H, W, C), dtype=f32)
    return q, k, v, res, g


# =================================================================== the slot layout ============================================
def col_index(H):
    """[H, H - 1]: the column members i of the pixels of row y, ascending, i != y"""
    c = np.arange(H - 1)[None, :]
    return c + (c >= np.arange(H)[:, None])


def to_slots(row, col):
    """row [N, H, W, W] (pixel (y, x), member (y, j)), col [N, H, W, H] (member (i, x); the entry i == y is dropped) -> [N, H, W, L]"""
    lib = torch if torch.is_tensor(row) else np
    H = row.shape[1]
    idx = col_index(H)[None, :, None, :]
    if lib is torch:
        idx = torch.from_numpy(idx).expand(col.shape[0], H, col.shape[2], H - 1)
        return torch.cat((row, torch.gather(col, 3, idx)), 3)
    return np.concatenate((row, np.take_along_axis(col, idx, 3)), 3)


def from_slots(a):
    """[N, H, W, L] -> row [N, H, W, W], col [N, H, W, H] with 0 at i == y"""
    lib = torch if torch.is_tensor(a) else np
    N, H, W, _ = a.shape
    row = a[..., :W]
    idx = col_index(H)[None, :, None, :]
    if lib is torch:
        col = torch.zeros((N, H, W, H), dtype=a.dtype)
        col.scatter_(3, torch.from_numpy(idx).expand(N, H, W, H - 1), a[..., W:])
        return row, col
    col = np.zeros((N, H, W, H), dtype=a.dtype)
    np.put_along_axis(col, np.broadcast_to(idx, (N, H, W, H - 1)), a[..., W:], 3)
    return row, col


# =================================================================== the plain formulas, on rows and columns (torch, any dtype) ==
def _lt(a):
    """rows <-> columns: [N, H, W, *] -> [N, W, H, *]"""
    return a.permute(0, 2, 1, 3)


def _sw(a):
    return a.transpose(2, 3)


def dots(a, b):
    """-> [N, H, W, L]: a[p] . b[m] for every member of every cross"""
    return to_slots(a @ _sw(b), _lt(_lt(a) @ _sw(_lt(b))))


def mix(wt, x):
    """-> [N, H, W, C]: sum_{m in X(p)} wt[p, m] x[m]"""
    row, col = from_slots(wt)
    return row @ x + _lt(_lt(col) @ _lt(x))


def mix_t(wt, x):
    """-> [N, H, W, C]: sum_{p in X(m)} wt[p, m] x[p], the weight the SOURCE p gives to the target m"""
    row, col = from_slots(wt)
    return _sw(row) @ x + _lt(_sw(_lt(col)) @ _lt(x))


def T(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t if dtype is None else t.to(dtype)


def plain_fwd(q, k, v, res, gamma, scale, dtype=torch.float64):
    """-> (w, out) as numpy arrays of dtype; res may be None"""
    q, k, v = (T(t, dtype) for t in (q, k, v))
    w = torch.softmax(dots(q, k) * float(f32(scale)), 3)
    out = float(f32(gamma)) * mix(w, v)
    if res is not None:
        out = T(res, dtype) + out
    return w.numpy(), out.numpy()


def plain_bwd(g, w, q, k, v, gamma, scale, dtype=torch.float64):
    """w: the forward's output as handed to the kernel -> dict(dq, dk, dv, dgamma)"""
    g, w, q, k, v = (T(t, dtype) for t in (g, w, q, k, v))
    ga, sc = float(f32(gamma)), float(f32(scale))
    t = dots(g, v)
    s = (w * t).sum(3, keepdim=True)
    e = sc * ga * w * (t - s)
    return dict(dq=mix(e, k).numpy(), dk=mix_t(e, q).numpy(), dv=(ga * mix_t(w, g)).numpy(), dgamma=s.sum().reshape(1).numpy())


def dense64(q, k, v, res, gamma, scale, g):
    """torch's float64 autograd of the dense masked attention -> dict(w [N, H, W, L], out, dq, dk, dv, dres, dgamma)"""
    N, H, W, D = q.shape
    qt, kt, vt, rt = (T(t, torch.float64).reshape(N, H * W, -1).requires_grad_(True) for t in (q, k, v, res))
    gm = torch.tensor(float(f32(gamma)), dtype=torch.float64, requires_grad=True)
    yy, xx = np.divmod(np.arange(H * W), W)
    cross = torch.from_numpy((yy[:, None] == yy[None, :]) | (xx[:, None] == xx[None, :]))
    s = (float(f32(scale)) * (qt @ kt.transpose(1, 2))).masked_fill(~cross, float("-inf"))
    wd = torch.softmax(s, 2)
    out = rt + gm * (wd @ vt)
    (out * T(g, torch.float64).reshape(N, H * W, -1)).sum().backward()
    # the dense weights in the slot layout
    my = np.concatenate((np.broadcast_to(yy[:, None], (H * W, W)), col_index(H)[yy]), 1)
    mx = np.concatenate((np.broadcast_to(np.arange(W)[None, :], (H * W, W)), np.broadcast_to(xx[:, None], (H * W, H - 1))), 1)
    w = wd.detach().numpy()[:, np.arange(H * W)[:, None], my * W + mx].reshape(N, H, W, H + W - 1)
    r = dict(w=w, out=out.detach().numpy().reshape(v.shape), dgamma=gm.grad.reshape(1).numpy())
    r.update(dq=qt.grad.numpy().reshape(q.shape), dk=kt.grad.numpy().reshape(q.shape), dv=vt.grad.numpy().reshape(v.shape),
             dres=rt.grad.numpy().reshape(v.shape))
    return r


# =================================================================== float64 references with their units ========================
def dot_count(D):
    return D


def lane_count(L):
    return cdiv(L, LCHUNK) - 1


def sum_count(P):
    return cdiv(P, SUM_THREADS) + 31 + 31


def cc_fwd64(q, k, v, res, gamma, scale):
    """-> dict(w, out, unit_out, arg [N, H, W, L], floor_out)"""
    w, out = plain_fwd(q, k, v, res, gamma, scale)
    D = q.shape[3]
    sc, ga = f64(f32(scale)), f64(f32(gamma))
    qt, kt, av = T(q, torch.float64), T(k, torch.float64), T(np.abs(v), torch.float64)
    u = (sc * dots(qt, kt)).numpy()
    a = abs(sc) * dots(qt.abs(), kt.abs()).numpy() * (dot_count(D) + 1)
    arg = a + a.max(3, keepdims=True) + np.abs(u - u.max(3, keepdims=True))
    unit = abs(ga) * mix(T(w), av).numpy() + (0.0 if res is None else np.abs(np.asarray(res, dtype=f64)))
    return dict(w=w, out=out, unit_out=unit, arg=arg, floor_out=TINY * abs(ga) * mix(torch.ones(w.shape, dtype=torch.float64), av).numpy())


def cc_bwd64(g, w, q, k, v, gamma, scale):
    """w: the forward's output as handed to the kernel -> dict(dq, dk, dv, dgamma, unit_*, floor_*)"""
    r = plain_bwd(g, w, q, k, v, gamma, scale)
    sg, ga = abs(f64(f32(scale)) * f64(f32(gamma))), abs(f64(f32(gamma)))
    wt, ag, aq, ak = T(w, torch.float64), T(np.abs(g), torch.float64), T(np.abs(q), torch.float64), T(np.abs(k), torch.float64)
    A = dots(ag, T(np.abs(v), torch.float64))
    mag = sg * (A + (wt * A).sum(3, keepdim=True))
    a, one = wt * mag, torch.ones(w.shape, dtype=torch.float64)
    r.update(unit_dq=mix(a, ak).numpy(), unit_dk=mix_t(a, aq).numpy(), unit_dv=ga * mix_t(wt, ag).numpy(),
             unit_dgamma=(wt * A).sum().reshape(1).numpy(),
             floor_dq=TINY * mix(1.0 + mag, ak).numpy(), floor_dk=TINY * mix_t(1.0 + mag, aq).numpy(),
             floor_dv=TINY * ga * mix_t(one, ag).numpy(), floor_dgamma=TINY * (1.0 + A).sum().reshape(1).numpy())
    return r


def _b(derived, cal, arg=0.0):
    return np.minimum(derived, CAL_MARGIN * cal * (1.0 + arg))


def cc_fwd_excess(got_w, got_out, q, k, v, res, gamma, scale):
    """-> (excess of w, excess of out)"""
    r = cc_fwd64(q, k, v, res, gamma, scale)
    L = r["w"].shape[3]
    e = 2.0 + r["arg"]
    cw = e + (r["w"] * e).sum(3, keepdims=True) + lane_count(L) + 6 + 1
    ew = rel_excess(got_w, r["w"], EPS * _b(cw, CAL["w"], r["arg"]) * r["w"] + TINY)
    co = L + 1 + cw.max(3, keepdims=True)
    eo = rel_excess(got_out, r["out"], EPS * _b(co, CAL["out"], r["arg"].max(3, keepdims=True)) * r["unit_out"] + r["floor_out"])
    return ew, eo


def bwd_counts(N, H, W, C):
    L = H + W - 1
    E = 2 * dot_count(C) + lane_count(L) + 11
    return dict(dq=E + L, dk=E + L, dv=L + 1, dgamma=dot_count(C) + lane_count(L) + 7 + sum_count(N * H * W))


def cc_bwd_excess(got, g, w, q, k, v, gamma, scale):
    """got: dict with any of dq, dk, dv, dgamma -> dict of excesses"""
    r = cc_bwd64(g, w, q, k, v, gamma, scale)
    N, H, W, C = v.shape
    cnt = bwd_counts(N, H, W, C)
    return {n: rel_excess(got[n], r[n], EPS * _b(cnt[n], CAL[n]) * r["unit_" + n] + r["floor_" + n]) for n in got}


# =================================================================== numpy fp32 emulations of the kernels' own order ============
FAULTS_FWD = ("centre_twice", "swapped", "no_max", "no_scale")
FAULTS_BWD = ("no_scale", "no_s", "dk_wrong_w", "dv_wrong_w", "dv_no_gamma", "e_no_gamma", "dgamma_one_image")


def emu_dots(a, b):
    """k_cc_dots: one fma chain over the channels from 0.0f -> row [N, H, W, W], col [N, H, W, H] (the entry i == y is not a slot)"""
    N, H, W, Dl = a.shape
    row, col = np.zeros((N, H, W, W), dtype=f32), np.zeros((N, H, W, H), dtype=f32)
    for d in range(Dl):
        row = fma(a[:, :, :, None, d], b[:, :, None, :, d], row)                     # pixel (y, x), member (y, j)
        col = fma(a[:, :, :, None, d], b[:, :, :, d].transpose(0, 2, 1)[:, None, :, :], col)     # member (i, x)
    return row, col


def emu_mix(wt, x, centre_twice=False):
    """k_cc_mix, TR = false: acc = fma(wt[p, slot], x[member], acc) from 0.0f over the slots ascending -> [N, H, W, C]"""
    N, H, W, _ = wt.shape
    acc = np.zeros((N, H, W, x.shape[3]), dtype=f32)
    for j in range(W):
        acc = fma(wt[:, :, :, j, None], x[:, :, None, j, :], acc)
    ci = col_index(H)
    for c in range(H - 1):
        acc = fma(wt[:, :, :, W + c, None], x[:, ci[:, c]], acc)
    return acc


def emu_mix_t(wt, x):
    """k_cc_mix, TR = true: the sources (y, 0 .. W - 1), then (i, x), i != y, ascending, each with the weight IT gives to the target"""
    N, H, W, _ = wt.shape
    acc = np.zeros((N, H, W, x.shape[3]), dtype=f32)
    for j in range(W):
        acc = fma(wt[:, :, j, :W, None], x[:, :, None, j, :], acc)                   # the source (y, j) holds the target (y, x) in slot x
    for i in range(H):
        ys = np.array([y for y in range(H) if y != i], dtype=np.int64)
        if ys.size:                                                                  # the source (i, x): slots W .. L - 1 <-> the targets y != i
            acc[:, ys] = fma(wt[:, i, :, W:].transpose(0, 2, 1)[..., None], x[:, None, i, :, :], acc[:, ys])
    return acc


def lanes_of(a):
    """[..., L] -> [..., LREGS, 64]: lane l of register r holds slot 64 r + l, absent slots 0"""
    out = np.zeros(a.shape[:-1] + (LREGS * LCHUNK,), dtype=f32)
    out[..., :a.shape[-1]] = a
    return out.reshape(a.shape[:-1] + (LREGS, LCHUNK))


def emu_fwd(q, k, v, res, gamma, scale, fault=None):
    """u2pl_cc_attn_fwd_f32 -> (w, out).  Faults: centre_twice (the pixel itself also as a column member: L + 1 weights, the
    extra one folded into slot x), swapped (the map walked as W x H: row and column lengths swapped), no_max, no_scale"""
    N, H, W, D = q.shape
    if fault == "swapped":
        sw = [t.reshape(N, W, H, -1) for t in (q, k, v)] + [None if res is None else res.reshape(N, W, H, -1)]
        w, out = emu_fwd(*sw, gamma, scale)
        return w.reshape(N, H, W, -1), out.reshape(N, H, W, -1)
    row, col = emu_dots(q, k)
    u = to_slots(row, col)
    if fault == "centre_twice":
        u = np.concatenate((u, row[:, np.arange(H)[:, None], np.arange(W)[None, :], np.arange(W)[None, :]][..., None]), 3)
    with np.errstate(over="ignore", invalid="ignore"):
        if fault != "no_scale":
            u = (f32(scale) * u).astype(f32)
        mx = np.zeros(u.shape[:3] + (1,), dtype=f32) if fault == "no_max" else u.max(3, keepdims=True)
        e = np.exp((u - mx).astype(f32)).astype(f32)
        la = lanes_of(e[..., :H + W - 1])
        z = la[..., 0, :]
        for r in range(1, LREGS):
            z = (z + la[..., r, :]).astype(f32)
        z = wave_sum(z)[..., None]
        if fault == "centre_twice":
            z = (z + e[..., -1:]).astype(f32)
        w = (e / z).astype(f32)
        if fault == "centre_twice":
            w, extra = w[..., :-1].copy(), w[..., -1]
            ix = np.broadcast_to(np.arange(W)[None, None, :, None], (N, H, W, 1))
            np.put_along_axis(w, ix, (np.take_along_axis(w, ix, 3) + extra[..., None]).astype(f32), 3)
        acc = emu_mix(w, v)
        ga = f32(gamma)
        out = (ga * acc).astype(f32) if res is None else fma(ga, acc, res)
    return w, out


def emu_sum(s):
    """k_cc_sum: thread j adds s[j], s[j + 1024], ...; 32 group sums of 32 threads; the group sums ascending"""
    P = s.size
    pad = np.zeros(cdiv(P, SUM_THREADS) * SUM_THREADS, dtype=f32)
    pad[:P] = s.reshape(-1)
    acc = np.zeros(SUM_THREADS, dtype=f32)
    for row_ in pad.reshape(-1, SUM_THREADS):
        acc = (acc + row_).astype(f32)
    grp = acc.reshape(32, 32)
    a = grp[:, 0]
    for j in range(1, 32):
        a = (a + grp[:, j]).astype(f32)
    tot = a[0]
    for j in range(1, 32):
        tot = f32(tot + a[j])
    return np.array([tot], dtype=f32)


def emu_bwd(g, w, q, k, v, gamma, scale, fault=None):
    """u2pl_cc_attn_bwd_f32 -> dict(dq, dk, dv, dgamma).  Faults: no_scale, no_s (the - s[p] term dropped), dk_wrong_w / dv_wrong_w
    (the gather takes w[m, p], the weight the target gives to the source), dv_no_gamma, e_no_gamma, dgamma_one_image"""
    t = to_slots(*emu_dots(g, v))
    lw, lt = lanes_of(w), lanes_of(t)
    s = (lw[..., 0, :] * lt[..., 0, :]).astype(f32)
    for r in range(1, LREGS):
        s = fma(lw[..., r, :], lt[..., r, :], s)
    s = wave_sum(s)
    ga = f32(gamma)
    sg = f32(1.0) if fault == "no_scale" else f32(scale)
    sg = sg if fault == "e_no_gamma" else f32(sg * ga)
    diff = t if fault == "no_s" else (t - s[..., None]).astype(f32)
    e = ((sg * w).astype(f32) * diff).astype(f32)
    dv = (emu_mix if fault == "dv_wrong_w" else emu_mix_t)(w, g)
    return dict(dq=emu_mix(e, k), dk=(emu_mix if fault == "dk_wrong_w" else emu_mix_t)(e, q),
                dv=dv if fault == "dv_no_gamma" else (ga * dv).astype(f32), dgamma=emu_sum(s[:1] if fault == "dgamma_one_image" else s))


# =================================================================== the ceilings ===============================================
def _ratio(got, ref, unit, arg=0.0, floor=0.0):
    return rel_excess(got, ref, EPS * (1.0 + arg) * np.asarray(unit, dtype=f64) + floor + 1e-300)


def case_gamma(HW):
    return -0.8 if (HW[0] + HW[1]) % 2 else 0.6


def measure(form="torch"):
    """-> {output: largest error in EPS (1 + arg) unit} over CAL_HW x CAL_NDC x FAMILIES"""
    worst = dict.fromkeys(CAL, 0.0)

    def up(n, val):
        worst[n] = max(worst[n], val)
    for HW in CAL_HW:
        for (N, D, C), fam in ((ndc, fam) for ndc in CAL_NDC for fam in FAMILIES):
            q, k, v, res, g = cc_case(N, HW, D, C, fam)
            sc, ga = case_scale(D), case_gamma(HW)
            r = cc_fwd64(q, k, v, res, ga, sc)
            w, out = plain_fwd(q, k, v, res, ga, sc, torch.float32) if form == "torch" else emu_fwd(q, k, v, res, ga, sc)
            up("w", _ratio(w, r["w"], r["w"], r["arg"], TINY))
            up("out", _ratio(out, r["out"], r["unit_out"], r["arg"].max(3, keepdims=True), r["floor_out"]))
            w32 = r["w"].astype(f32)
            b = cc_bwd64(g, w32, q, k, v, ga, sc)
            got = plain_bwd(g, w32, q, k, v, ga, sc, torch.float32) if form == "torch" else emu_bwd(g, w32, q, k, v, ga, sc)
            for n in OUTS_BWD:
                up(n, _ratio(got[n], b[n], b["unit_" + n], 0.0, b["floor_" + n]))
    return worst
