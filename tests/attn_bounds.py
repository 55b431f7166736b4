"""Float64 references, numpy fp32 emulations, shape tables and error bounds of the dense attention kernels in
u2pl_amd/csrc/attn.hip (u2pl_attn_{fwd,bwd}_f32), shared by tests/test_attn_cpu.py and tests/test_gpu_attn.py.  Not a conftest:
imported by name, like cc_bounds.

Arrays are rows: q, dq [N, Pq, heads*D]; k, dk [N, Pk, heads*D]; v, dv [N, Pk, heads*Dv]; o, g [N, Pq, heads*Dv]; head h owns the
columns h*D .. / h*Dv ..; lse [N, heads, Pq].  scale is a float.  The backward references take the forward's saved o and lse as
the inputs they are for the kernel: the fp32 values handed to the kernel are the values the float64 formula is evaluated on.

The float64 reference is torch's autograd of the dense formula softmax(scale q k^T) v (dense64); plain_fwd / plain_bwd state the
kernels' formulas (lse = logsumexp, P = exp(S - lse), delta = g . o, dS = P (dP - delta)) in a dtype of choice: in float64 they are
what the bounds are taken against (tests/test_attn_cpu.py holds them to dense64 in every score family), in float32 they are
"torch's own fp32 arithmetic of the plain formulas" that the ceilings are measured from.

Every element is held to  |got - ref64| <= EPS min(derived, CAL_MARGIN measured (1 + arg)) unit + floor  (EPS = 2^-24, one unit
per fp32 rounding; CAL_MARGIN of contrast_bounds).

  units     o: sum_j P |v|;  lse: 1 + |lse|;  dv: sum_p P[p, j] |g[p]|;  with A[p, j] = sum_c |g[p]||v[j]| and
            a = |scale| P (A + sum_j P A):  dq: sum_j a[p, j] |k[j]|,  dk: sum_p a[p, j] |q[p]|.
  arg       the rounding of an exponent's argument, in units of EPS, is a RELATIVE error of the exponential (ocr_bounds, cc_bounds):
            u = scale dot (error a_j = (dot_count(D) + 1) |scale| sum |q||k|), the reference point (the running maximum, an u
            itself: max_j a_j; the backward's lse is an input), the subtraction |u - mx| resp. |u - lse|:
            forward arg = a_j + max_j a_j + |u - mx|;  backward arg = a_j + |u - lse|.  An output takes the largest arg of the
            weights it sums.
  derived   roundings read off the straight-line code of attn.hip; expf and logf count as 2.  T = ceil(Pk / BK) key tiles.
            o:   a weight: 2 + arg; ONE rounding per later key-tile rescale: T; the chain over the keys: Pk; the same for Z with
                 ceil(Pk / 4) adds of a lane and 2 across the lanes; one division:
                 2 (2 + arg) + 2 T + Pk + ceil(Pk / 4) + 3.
                 (alpha = expf(m - m') multiplies the sums of o and of Z alike: its own error cancels in o.)
            lse: it does not cancel here: 3 + |m - m'| per tile, sum |m - m'| <= max u - min u = range:
                 2 max a + 2 + max |u - mx| + 3 T + range + ceil(Pk / 4) + 2 + 2 (logf) + 1.
            dS = P (dP - delta): P: 2 + arg (+ the scale product, in a); dP and delta: dot_count(Dv) each, relative to A and to
                 sum P A; the subtraction and the product: 2.   E = 4 + arg + dot_count(Dv).
            dq: E + Pk + 1 (scale).   dk: E + Pq + NS + 1 (NS slab partials).   dv: 2 + arg + Pq + NS.
  floor     a result below 2^-126 may be flushed to zero by expf or by a product: every weight (and dS) is allowed an absolute
            error of 2^-126, which every output sees multiplied by the magnitude of what the weight multiplies (floor_*).
  measured  what torch's own fp32 CPU arithmetic of the plain formulas (plain_*(..., torch.float32)) reaches against float64 over
            CAL_PAIRS x CAL_NHDD x FAMILIES, in units of EPS (1 + arg) unit -- never a HIP kernel (python -m pytest
            tests/test_attn_cpu.py -s -k ceilings; the emulation of the kernels' order in brackets):
                o   0.970 [0.815]    lse 0.153 [0.153]    dq  0.074 [0.130]    dk  0.337 [0.174]    dv  0.400 [0.426]
            (arg carries dot_count + 1 roundings of |scale| sum |q||k| per score: at D = 20 the figures are small; the largest come
            from D = 4, where the roundings of the sums over the keys are what is left.)

The emulations restate the kernels' order in numpy fp32 (fma as one rounding of the float64 product-sum): the channel order of a
dot chain, the key tiles ascending, the permuted key order 16 t + 4 s + r inside an MFMA step, the online rescale, the per-lane
sums of Z and their pairing, the slab finish.  np.exp / np.log stand for expf / logf (they differ by an ulp at most: the
emulation is held to the bounds, not to the kernel's bits)."""
import numpy as np
import torch

from contrast_bounds import CAL_MARGIN
from glue_bounds import SENTINEL_BITS, bits_equal, rel_excess  # noqa: F401
from ocr_bounds import cdiv, fma, sentinel  # noqa: F401
from split_bounds import EPS

f32, f64 = np.float32, np.float64

# csrc/attn.hip
BQ = 64                         # ATTN_BQ: owned rows of a block (queries of k_attn_fwd / k_attn_dq, keys of k_attn_kgrad)
BK = 64                         # ATTN_BK: walked rows of one tile
DVC = 128                       # ATTN_DVC: channels of one mix pass
MAX_D, MAX_DV = 128, 512        # ATTN_MAX_D, ATTN_MAX_DV
GRID_CAP = 4096                 # ATTN_MAX_BLOCKS
FILL = 512                      # ATTN_FILL
SLAB_MIN = 256                  # ATTN_SLAB_MIN
MAX_SLABS = 32                  # ATTN_MAX_SLABS
TINY = 2.0 ** -126


def slabs(N, heads, Pq, Pk):
    """attn_slabs -> (NS, rows)"""
    tiles = N * heads * cdiv(Pk, BQ)
    ns = max(1, min(cdiv(FILL, tiles), cdiv(Pq, SLAB_MIN), MAX_SLABS))
    rows = cdiv(cdiv(Pq, ns), BK) * BK
    return cdiv(Pq, rows), rows


def bwd_ws_floats(N, heads, Pq, Pk, D, Dv):
    NS = slabs(N, heads, Pq, Pk)[0]
    return cdiv(N * heads * Pq, 4) * 4 + (NS * N * Pk * heads * (D + Dv) if NS > 1 else 0)


# the first Pq that opens a second query slab beside Pk = 3 (one key tile per image and head)
SLAB_PQ = SLAB_MIN + 1
PAIRS = ((1, 1), (1, 7), (7, 1), (3, 5), (BQ - 1, BK - 1), (BQ, BK), (BQ + 1, BK + 1), (2 * BQ + 3, 2 * BK + 5), (BQ + 1, 1),
         (1, 2 * BK + 5), (SLAB_PQ, 3))
NHDD = ((1, 1, 4, 4), (1, 1, 128, 4), (3, 2, 20, 36), (2, 3, 64, 260), (1, 1, 64, 512))        # (N, heads, D, Dv)
assert slabs(1, 1, SLAB_PQ, 3)[0] == 2 and slabs(1, 1, SLAB_PQ - 1, 3)[0] == 1 and slabs(3, 2, SLAB_PQ, 3)[0] == 2
ONLINE_PAIR = (BQ + 1, 16 * BK + 1)
FAMILIES = ("normal", "big", "const")            # scores N(0, 2) / +-100 / every key the same
ONLINE_FAMILIES = ("first", "last", "ascending")  # the row maximum in the first key tile / in the last / rising in every tile
# every kernel takes a second trip of its grid-stride loop: k_attn_fwd, k_attn_dq, k_attn_kgrad (one block an item) at 4097 images
# of one query and one key; k_attn_delta (256 rows a block) at 4097 x 257 rows; k_attn_finish (256 floats a block) at
# 2049 keys x 512 value channels in 2 slabs
GRID_CASES = ((4097, 1, 1, 1, 4, 4), (4097, 1, SLAB_PQ, 1, 4, 4), (1, 1, SLAB_PQ, 2049, 4, 512))    # (N, heads, Pq, Pk, D, Dv)
assert 4097 > GRID_CAP and 4097 * SLAB_PQ > GRID_CAP * 256 and 2049 * 512 > GRID_CAP * 256 and slabs(1, 1, SLAB_PQ, 2049)[0] == 2
CAL_PAIRS = ((1, 1), (1, 7), (7, 1), (3, 5), (33, 70), (70, 33), (130, 9))
CAL_NHDD = ((3, 2, 20, 20), (1, 1, 4, 4))

# ---- calibrated ceilings: torch's own fp32 arithmetic against float64 (never the HIP kernels), rounded up by a few per cent
CAL = dict(o=1.0, lse=0.16, dq=0.078, dk=0.35, dv=0.42)
OUTS_BWD = ("dq", "dk", "dv")


def case_scale(D):
    """so that q . k of standard normal rows has the variance 2: the score family N(0, 2)"""
    return float(np.sqrt(2.0 / D))


def attn_case(N, heads, Pq, Pk, D, Dv, family="normal", seed=0):
    """-> q [N, Pq, heads*D], k [N, Pk, heads*D], v [N, Pk, heads*Dv], g [N, Pq, heads*Dv] (float32)"""
    fams = FAMILIES + ONLINE_FAMILIES
    rng = np.random.default_rng([seed, 53, N, heads, Pq, Pk, D, Dv, fams.index(family)])
    q = rng.standard_normal((N, Pq, heads, D), dtype=f32)
    k = rng.standard_normal((N, Pk, heads, D), dtype=f32)
    if family == "big":
        q = (q * f32(100 / np.sqrt(2.0))).astype(f32)
    if family == "const":
        k[:] = k[:, :1]                          # every key the same: the weights are 1 / Pk
    if family in ONLINE_FAMILIES:                # the score is scale * q[0] * c[j]: q[0] > 0, the other channels of k are 0
        q[..., 0] = np.abs(q[..., 0]) + f32(0.5)
        k[..., 1:] = 0
        if family == "ascending":
            k[..., 0] = (np.arange(Pk, dtype=f32) * f32(0.03))[None, :, None] / f32(case_scale(D))
        else:
            k[..., 0] = np.clip(k[..., 0], -2, 2)
            k[:, min(3, Pk - 1) if family == "first" else Pk - 1, :, 0] = f32(6.0 / case_scale(D))
    v = rng.standard_normal((N, Pk, heads * Dv), dtype=f32) + f32(0.5)
    g = rng.standard_normal((N, Pq, heads * Dv), dtype=f32)
    return q.reshape(N, Pq, heads * D), k.reshape(N, Pk, heads * D), v, g


# =================================================================== the plain formulas (torch, any dtype) ======================
def T(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t if dtype is None else t.to(dtype)


def hd(a, heads):
    """[N, P, heads*W] -> [N, heads, P, W] (numpy or torch)"""
    N, P, HW = a.shape
    a = a.reshape(N, P, heads, HW // heads)
    return a.permute(0, 2, 1, 3) if torch.is_tensor(a) else a.transpose(0, 2, 1, 3)


def un(a):
    """[N, heads, P, W] -> [N, P, heads*W]"""
    N, H, P, W = a.shape
    a = a.permute(0, 2, 1, 3) if torch.is_tensor(a) else a.transpose(0, 2, 1, 3)
    return a.reshape(N, P, H * W)


def plain_fwd(q, k, v, heads, scale, dtype=torch.float64):
    """-> (o [N, Pq, heads*Dv], lse [N, heads, Pq]) as numpy arrays of dtype"""
    q, k, v = (hd(T(t, dtype), heads) for t in (q, k, v))
    S = float(f32(scale)) * (q @ k.transpose(2, 3))
    lse = torch.logsumexp(S, 3)
    return un(torch.exp(S - lse[..., None]) @ v).numpy(), lse.numpy()


def plain_bwd(g, q, k, v, o, lse, heads, scale, dtype=torch.float64):
    """o, lse: the forward's outputs as handed to the kernel -> dict(dq, dk, dv)"""
    g, q, k, v, o = (hd(T(t, dtype), heads) for t in (g, q, k, v, o))
    sc = float(f32(scale))
    P = torch.exp(sc * (q @ k.transpose(2, 3)) - T(lse, dtype)[..., None])
    dS = P * (g @ v.transpose(2, 3) - (g * o).sum(3, keepdim=True))
    return dict(dq=un(sc * (dS @ k)).numpy(), dk=un(sc * (dS.transpose(2, 3) @ q)).numpy(), dv=un(P.transpose(2, 3) @ g).numpy())


def dense64(q, k, v, heads, scale, g):
    """torch's float64 autograd of the dense formula -> dict(o, lse, dq, dk, dv)"""
    qt, kt, vt = (T(t, torch.float64).requires_grad_(True) for t in (q, k, v))
    S = float(f32(scale)) * (hd(qt, heads) @ hd(kt, heads).transpose(2, 3))
    o = un(torch.softmax(S, 3) @ hd(vt, heads))
    (o * T(g, torch.float64)).sum().backward()
    mx = S.detach().max(3, keepdim=True).values
    lse = (mx + torch.log(torch.exp(S.detach() - mx).sum(3, keepdim=True)))[..., 0]
    return dict(o=o.detach().numpy(), lse=lse.numpy(), dq=qt.grad.numpy(), dk=kt.grad.numpy(), dv=vt.grad.numpy())


# =================================================================== float64 references with their units ========================
def dot_count(W):
    return W


def _scores64(q, k, heads, scale):
    """-> u [N, heads, Pq, Pk], a (the error of u in units of EPS)"""
    D = q.shape[2] // heads
    sc = f64(f32(scale))
    qh, kh = hd(np.asarray(q, dtype=f64), heads), hd(np.asarray(k, dtype=f64), heads)
    u = sc * (qh @ kh.transpose(0, 1, 3, 2))
    a = abs(sc) * (np.abs(qh) @ np.abs(kh).transpose(0, 1, 3, 2)) * (dot_count(D) + 1)
    return u, a


def attn_fwd64(q, k, v, heads, scale):
    """-> dict(o, lse, unit_o, arg [N, heads, Pq] (the largest of the row), rng, amax, floor_o)"""
    o, lse = plain_fwd(q, k, v, heads, scale)
    u, a = _scores64(q, k, heads, scale)
    mx = u.max(3, keepdims=True)
    arg = (a + a.max(3, keepdims=True) + np.abs(u - mx)).max(3)
    av = hd(np.abs(np.asarray(v, dtype=f64)), heads)
    P = np.exp(u - lse[..., None])
    return dict(o=o, lse=lse, unit_o=un(P @ av), arg=arg, rng=(mx[..., 0] - u.min(3)), amax=a.max(3),
                dev=np.abs(u - mx).max(3), floor_o=TINY * un(np.broadcast_to(av.sum(2, keepdims=True), P.shape[:3] + av.shape[3:])))


def attn_bwd64(g, q, k, v, o, lse, heads, scale):
    """o, lse: as handed to the kernel -> dict(dq, dk, dv, unit_*, floor_*, arg [N, heads, Pq, Pk])"""
    r = plain_bwd(g, q, k, v, o, lse, heads, scale)
    sc = abs(f64(f32(scale)))
    u, a = _scores64(q, k, heads, scale)
    l64 = np.asarray(lse, dtype=f64)[..., None]
    P = np.exp(u - l64)
    ag, aq, ak, av = (hd(np.abs(np.asarray(t, dtype=f64)), heads) for t in (g, q, k, v))
    A = ag @ av.transpose(0, 1, 3, 2)
    mag = sc * (A + (P * A).sum(3, keepdims=True))
    w = P * mag
    tr = lambda x: x.transpose(0, 1, 3, 2)      # noqa: E731
    r.update(arg=a + np.abs(u - l64), unit_dq=un(w @ ak), unit_dk=un(tr(w) @ aq), unit_dv=un(tr(P) @ ag),
             floor_dq=TINY * un((1.0 + mag) @ ak), floor_dk=TINY * un(tr(1.0 + mag) @ aq),
             floor_dv=TINY * un(np.broadcast_to(ag.sum(2, keepdims=True), (ag.shape[0], ag.shape[1], P.shape[3], ag.shape[3]))))
    return r


def _b(derived, cal, arg=0.0):
    return np.minimum(derived, CAL_MARGIN * cal * (1.0 + arg))


def _rows(x, heads, width):
    """a per-(image, head, row) figure [N, heads, P] -> one per element of [N, P, heads*width]"""
    return un(np.broadcast_to(x[..., None], x.shape + (width,)))


def attn_fwd_excess(got_o, got_lse, q, k, v, heads, scale):
    """-> (excess of o, excess of lse)"""
    r = attn_fwd64(q, k, v, heads, scale)
    Pk, Dv = k.shape[1], v.shape[2] // heads
    Tn = cdiv(Pk, BK)
    co = 2 * (2.0 + r["arg"]) + 2 * Tn + Pk + cdiv(Pk, 4) + 3
    eo = rel_excess(got_o, r["o"], EPS * _rows(_b(co, CAL["o"], r["arg"]), heads, Dv) * r["unit_o"] + r["floor_o"])
    cl = 2 * r["amax"] + 2 + r["dev"] + 3 * Tn + r["rng"] + cdiv(Pk, 4) + 5
    el = rel_excess(got_lse, r["lse"], EPS * _b(cl, CAL["lse"], r["arg"]) * (1.0 + np.abs(r["lse"])))
    return eo, el


def attn_bwd_excess(got, g, q, k, v, o, lse, heads, scale):
    """got: dict with any of dq, dk, dv -> dict of excesses"""
    r = attn_bwd64(g, q, k, v, o, lse, heads, scale)
    N, Pq, Pk = q.shape[0], q.shape[1], k.shape[1]
    D, Dv = q.shape[2] // heads, v.shape[2] // heads
    NS = slabs(N, heads, Pq, Pk)[0]
    aq, ak = r["arg"].max(3), r["arg"].max(2)             # per query, per key
    E = 4.0 + dot_count(Dv)
    cnt = dict(dq=(E + aq + Pk + 1, aq, D), dk=(E + ak + Pq + NS + 1, ak, D), dv=(2.0 + ak + Pq + NS, ak, Dv))
    return {n: rel_excess(got[n], r[n], EPS * _rows(_b(cnt[n][0], CAL[n], cnt[n][1]), heads, cnt[n][2]) * r["unit_" + n] + r["floor_" + n])
            for n in got}


# =================================================================== numpy fp32 emulations of the kernels' own order ============
FAULTS_FWD = ("pad_scored_zero", "no_rescale", "lse_max_only", "heads_swapped", "perm_p_not_v", "rows_past_pq")
FAULTS_BWD = ("delta_wrong_head", "dk_no_scale", "dq_scale_twice", "no_delta", "last_slab_dropped")


def emu_dots(a, b):
    """attn_dots: [..., R, W] x [..., C, W] -> [..., R, C]; the chain c0 = 0, 16, ..; x = 0 .. 3; s = 0 .. 3: channel c0 + 4 s + x"""
    W = a.shape[-1]
    acc = np.zeros(a.shape[:-1] + (b.shape[-2],), dtype=f32)
    for c0 in range(0, W, 16):
        for x in range(4):
            for s in range(4):
                c = c0 + 4 * s + x
                if c < W:
                    acc = fma(a[..., :, None, c], b[..., None, :, c], acc)
    return acc


def tile_order(n, natural=False):
    """the walked rows of one tile (n <= 64 of them are real) in the order of the mix chain: t, r, s -> 16 t + 4 s + r"""
    order = [16 * t + (4 * r + s if natural else 4 * s + r) for t in range(4) for r in range(4) for s in range(4)]
    return [j for j in order if j < n]


def emu_mix(w, x, r0, r1):
    """attn_mix over the walked rows r0 .. r1: w [..., R (walked), C (owned)], x [..., R, W] -> [..., C, W] from 0.0f"""
    acc = np.zeros(w.shape[:-2] + (w.shape[-1], x.shape[-1]), dtype=f32)
    for t0 in range(r0, r1, BK):
        for j in tile_order(min(BK, r1 - t0)):
            acc = fma(w[..., t0 + j, :, None], x[..., t0 + j, None, :], acc)
    return acc


def emu_fwd(q, k, v, heads, scale, fault=None):
    """u2pl_attn_fwd_f32 -> (o [N, Pq, heads*Dv], lse [N, heads, Pq]).  Faults: pad_scored_zero (the padding keys of the last tile
    scored 0 instead of excluded), no_rescale (the sums are not rescaled when the running maximum rises), lse_max_only,
    heads_swapped (head h reads the values of head heads - 1 - h), perm_p_not_v (the permuted key order of an MFMA step applied
    to P, V loaded in natural order), rows_past_pq (the rows of the last query tile past Pq written: o gets BQ-aligned rows)"""
    qh, kh, vh = hd(q, heads), hd(k, heads), hd(v, heads)
    if fault == "heads_swapped":
        vh = vh[:, ::-1]
    N, H, Pq, _ = qh.shape
    Pk, Dv = kh.shape[2], vh.shape[3]
    sc = f32(scale)
    S = emu_dots(kh, qh)                                       # [.., Pk (walked), Pq (owned)]
    m = np.full((N, H, Pq), -np.inf, dtype=f32)
    z = np.zeros((N, H, Pq, 4), dtype=f32)
    acc = np.zeros((N, H, Pq, Dv), dtype=f32)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for k0 in range(0, Pk, BK):
            n = min(BK, Pk - k0)
            u = (sc * S[:, :, k0:k0 + n]).astype(f32)          # [.., n, Pq]
            vt = vh[:, :, k0:k0 + n]
            if fault == "pad_scored_zero" and n < BK:
                u = np.concatenate((u, np.zeros((N, H, BK - n, Pq), dtype=f32)), 2)
                vt = np.concatenate((vt, np.zeros((N, H, BK - n, Dv), dtype=f32)), 2)
                n = BK
            mn = np.maximum(m, u.max(2))
            alpha = np.exp((m - mn).astype(f32)).astype(f32)
            if fault == "no_rescale":
                alpha = np.ones_like(alpha)
            m = mn
            p = np.exp((u - mn[:, :, None, :]).astype(f32)).astype(f32)
            z = (z * alpha[..., None]).astype(f32)
            for t in range(4):
                for r in range(4):
                    for s in range(4):
                        j = 16 * t + 4 * s + r
                        if j < n:
                            z[..., s] = (z[..., s] + p[:, :, j]).astype(f32)
            acc = (acc * alpha[..., None]).astype(f32)
            for j, jn in zip(tile_order(BK), tile_order(BK, True)):
                if j < n:
                    if fault == "perm_p_not_v":
                        row = vt[:, :, jn] if jn < n else np.zeros_like(vt[:, :, 0])
                    else:
                        row = vt[:, :, j]
                    acc = fma(p[:, :, j, :, None], row[:, :, None, :], acc)
        Z = ((z[..., 0] + z[..., 1]).astype(f32) + (z[..., 2] + z[..., 3]).astype(f32)).astype(f32)
        o = (acc / Z[..., None]).astype(f32)
        lse = m if fault == "lse_max_only" else (m + np.log(Z).astype(f32)).astype(f32)
    o = un(o)
    if fault == "rows_past_pq":
        o = np.concatenate((o, np.zeros((N, cdiv(Pq, 16) * 16 - Pq, o.shape[2]), dtype=f32)), 1)
    return o, lse


def emu_bwd(g, q, k, v, o, lse, heads, scale, fault=None):
    """u2pl_attn_bwd_f32 -> dict(dq, dk, dv).  Faults: delta_wrong_head (delta taken over the next head's columns), dk_no_scale,
    dq_scale_twice, no_delta (dS = P dP), last_slab_dropped (the slab partials added in the wrong count)"""
    gh, qh, kh, vh, oh = (hd(t, heads) for t in (g, q, k, v, o))
    N, H, Pq, _ = qh.shape
    Pk, Dv = kh.shape[2], vh.shape[3]
    sc = f32(scale)
    sh = 1 if fault == "delta_wrong_head" else 0
    delta = np.zeros((N, H, Pq), dtype=f32)
    for c in range(Dv):
        delta = fma(np.roll(gh, sh, 1)[..., c], np.roll(oh, sh, 1)[..., c], delta)
    with np.errstate(over="ignore", invalid="ignore"):
        S = emu_dots(qh, kh)                                   # [.., Pq, Pk]
        P = np.exp(((sc * S).astype(f32) - np.asarray(lse, dtype=f32)[..., None]).astype(f32)).astype(f32)
        dP = emu_dots(gh, vh)
        dS = (P * (dP if fault == "no_delta" else (dP - delta[..., None]).astype(f32))).astype(f32)
        tr = lambda x: np.ascontiguousarray(x.transpose(0, 1, 3, 2))      # noqa: E731
        dq = (sc * emu_mix(tr(dS), kh, 0, Pk)).astype(f32)
        if fault == "dq_scale_twice":
            dq = (sc * dq).astype(f32)
        NS, rows = slabs(N, H, Pq, Pk)
        parts_k, parts_v = [], []
        for s in range(NS):
            r0, r1 = s * rows, min(Pq, (s + 1) * rows)
            pk = emu_mix(dS, qh, r0, r1)
            parts_k.append(pk if fault == "dk_no_scale" else (sc * pk).astype(f32))
            parts_v.append(emu_mix(P, gh, r0, r1))
        if fault == "last_slab_dropped" and NS > 1:
            parts_k, parts_v = parts_k[:-1], parts_v[:-1]
        dk, dv = parts_k[0], parts_v[0]
        for pk, pv in zip(parts_k[1:], parts_v[1:]):
            dk, dv = (dk + pk).astype(f32), (dv + pv).astype(f32)
    return dict(dq=un(dq), dk=un(dk), dv=un(dv))


def frame_intact(rows, Pq):
    """rows [N, R, C]: what a call wrote for each image, R >= Pq rows of them, into a sentinel-framed [N * Pq + BQ, C] buffer the way
    the kernel addresses it (image n starts at row n * Pq) -> is the frame behind the last image intact?"""
    N, R, C = rows.shape
    buf = np.full((N * Pq + BQ, C), sentinel(), dtype=f32)
    for n in range(N):
        buf[n * Pq:n * Pq + R] = rows[n]
    return bool((buf[N * Pq:].view(np.uint32) == SENTINEL_BITS).all())


# =================================================================== the ceilings ===============================================
def _ratio(got, ref, unit, arg=0.0, floor=0.0):
    return rel_excess(got, ref, EPS * (1.0 + arg) * np.asarray(unit, dtype=f64) + floor + 1e-300)


def measure(form="torch"):
    """-> {output: largest error in EPS (1 + arg) unit} over CAL_PAIRS x CAL_NHDD x FAMILIES"""
    worst = dict.fromkeys(CAL, 0.0)

    def up(n, val):
        worst[n] = max(worst[n], val)
    for Pq, Pk in CAL_PAIRS:
        for (N, H, D, Dv), fam in ((c, fam) for c in CAL_NHDD for fam in FAMILIES):
            q, k, v, g = attn_case(N, H, Pq, Pk, D, Dv, fam)
            sc = case_scale(D)
            r = attn_fwd64(q, k, v, H, sc)
            o, lse = plain_fwd(q, k, v, H, sc, torch.float32) if form == "torch" else emu_fwd(q, k, v, H, sc)
            up("o", _ratio(o, r["o"], r["unit_o"], _rows(r["arg"], H, Dv), r["floor_o"]))
            up("lse", _ratio(lse, r["lse"], 1.0 + np.abs(r["lse"]), r["arg"]))
            o32, l32 = r["o"].astype(f32), r["lse"].astype(f32)
            b = attn_bwd64(g, q, k, v, o32, l32, H, sc)
            got = plain_bwd(g, q, k, v, o32, l32, H, sc, torch.float32) if form == "torch" else emu_bwd(g, q, k, v, o32, l32, H, sc)
            aq, ak = b["arg"].max(3), b["arg"].max(2)
            for n, (ar, wd) in dict(dq=(aq, D), dk=(ak, D), dv=(ak, Dv)).items():
                up(n, _ratio(got[n], b[n], b["unit_" + n], _rows(ar, H, wd), b["floor_" + n]))
    return worst
