"""Float64 references, an fp32 emulation in the kernels' stage order (with faults) and the error bounds of the Lovasz-Softmax
route (u2pl_amd/csrc/lovasz.hip), shared by tests/test_lovasz_cpu.py and tests/test_gpu_lovasz.py.  Not a conftest:
imported by name, like loss_bounds.

THE DEFINITION (restated in float64 by lovasz_ref; Berman, Triki, Blaschko, CVPR 2018, Algorithm 1 on the softmax errors):
    valid pixels: target != ignore, the batch flattened; for class c and valid pixel i  m_i(c) = |[y_i == c] - softmax(z_i)[c]|;
    pi sorts the valid pixels of c by m descending, ties in ascending flat pixel index (stable);
    fg_j = [y_pi_j == c], G = sum fg, F_j = sum_{k <= j} fg_k, I_j = G - F_j, U_j = G + (j - F_j)   (integers, exact);
    g_j = 1 / U_j (fg_j = 1);  I_j / ((U_j - 1) U_j) (fg_j = 0, G > 0);  [j == 1] (G == 0)   -- the closed form of J_j - J_{j-1};
    loss_c = sum_j m_pi_j g_j; loss = mean over the classes with G > 0 ("present"; 0 when there are none) or over all C classes;
    d loss / d p_i(c) = -/+ g_{pi^-1(i)} / n_classes (minus where y_i == c), through the softmax Jacobian to dz; 0 on ignored pixels.
lovasz_torch64 is its twin written the published way (torch.sort(stable=True), cumsum, Jaccard differences, autograd);
test_lovasz_cpu.py shows that the two agree in float64 (closed form against differences, analytic gradient against autograd).

THE EMULATION (emu_lovasz) follows the kernels stage by stage in numpy fp32: k_lv_errors' softmax (sequential fp32 sum, expf at
float64-rounded-once), keys 0x3F800000 - bits(m) and 0x3FFFFFFF on ignored pixels, payload pixel | fg << 31, a stable sort of the
keys chunk by chunk, the tile-wise foreground scan with its carries, g formed in double and rounded once, the per-lane sequential
fp32 sums of m g over the 32 rounds of a 2048-element tile, the xor butterfly over the 64 lanes, the slabs added in double lane-
strided and by the same butterfly, the classes upward; the backward with kf = out3[1] gout gmul in fp32.  FAULTS lists the wrong
emulations every check below must reject on at least one case of the grid (test_lovasz_cpu.py asserts it).

THE BOUNDS.  Units: EPS = 2^-24.
  keys     |m32 - m64| <= E_prob(C) of tests/loss_bounds.py (the same softmax pick; 1 - p is one more rounding of at most EPS / 2,
           inside the slack of the count); fg bits, G, the valid count: exact; every ignored key above every valid key.
  sort     exact: numpy's stable sort of the implementation's OWN keys, keys and payloads bit for bit.
  g        given the implementation's own permutation the scans are integers (exact) and g is one rounding of a double
           quotient: g_count = 1 unit of EPS g (2^-24 g is the half-ulp of a value just above a power of two).  Calibrated: CAL_LV_G below, times CAL_LV_MARGIN = 2.
  loss     the Lovasz extension is 1-Lipschitz in max|m| (g >= 0, sum g <= 1), so |L(m32) - L(m64)| <= E_prob(C); the summation
           adds sum_count = 2 (g, the product) + rounds per lane (<= 32) + 6 (butterfly) + 1 (the fp32 result) units of EPS on
           loss_c <= 1; the double finish is below 1e-3 units.  Calibrated: CAL_LV_SUM.  The smaller of count and calibration is
           added to E_prob; the README's 1e-4 max(1, |loss|) caps the whole.
  dz       in units of EPS kf A_i, A_i = max_c g[c][i] (so |a_c| <= kf A_i and |a_k - dot| <= 2 kf A_i): the error of p_k
           (prob_count, absolute) times 2; the error of dot: sum_c |a_c| dp_c <= kf A_i (prob_count + ln C) since
           sum_c p_c |d_c| <= ln C, its C - 1 sequential adds and one product each; 4 roundings in a_c (g, out3[1], gout, gmul);
           the subtraction and the product: dz_count = 3 prob_count + ln C + C + 6.  Calibrated: CAL_LV_DZ_A + CAL_LV_DZ_B sqrt(C).
The calibrated constants are ceilings measured ON THE CPU, never from a HIP kernel, over FAMILIES x CAL_IGNORES x both class modes
at CAL_SHAPE, from two fp32 forms: the emulation above and a torch-fp32 restatement (torch_lovasz_fp32: F.softmax, the closed
form in fp32 arithmetic, torch's pairwise fp32 sum, fp32 autograd); the larger of the two is the constant, and the asserted
bound allows CAL_LV_MARGIN = 2 over it (two fp32 orderings of the same sums differ by about that).  Measured (emulation / torch):

                 C = 2          C = 19         C = 21         C = 33          C = 150         C = 255
    g            0.99 / 0.99    1.00 / 1.00    1.00 / 1.00    1.00 / 1.00     1.00 / 1.00     1.00 / 1.00
    sum          0.58 / 0.55    0.64 / 1.20    0.73 / 2.15    0.68 / 1.68     0.85 / 1.82     0.67 / 1.96
    dz           2.78 / 2.74    6.74 / 6.74    6.69 / 6.69    7.65 / 7.65    14.92 / 14.92   22.26 / 22.26

(g: both forms round one quotient, integers below 2^24 are exact in fp32.  sum: torch's pairwise sum of the whole list against the
kernels' 32-deep lane sums and butterfly.  dz: the error of the softmax dominates and both forms share it; it grows like the CE
gradient's, CAL_GRAD of tests/loss_bounds.py.)
(python -m pytest tests/test_lovasz_cpu.py -s -k ceilings prints the table and asserts that the constants are ceilings of it.)"""
import math

import numpy as np
import torch
import torch.nn.functional as F

import loss_bounds as LB
from loss_bounds import CLASSES, FAMILIES, IGNORE, IGNORES, SHAPES, E_prob, apply_ignore, make_case  # noqa: F401
from split_bounds import EPS

f32, f64 = np.float32, np.float64
ONE_BITS = 0x3F800000
IGN_KEY = 0x3FFFFFFF
TILE = 2048                      # elements a wave orders / scans (u2pl_segsort_tile())
BINS = 256
DEFAULT_CHUNK = 32               # u2pl_lovasz_default_chunk()
ALIGN = 256
CONTRACT_LOSS = LB.CONTRACT_LOSS
MODES = ("present", "all")
CAL_SHAPE = (2, 23, 31)
CAL_IGNORES = ("none", "some", "image", "one")
CAL_LV_MARGIN = 2.0
# measured ceilings over the calibration grid at C = 2, 19, 21, 33, 150, 255 (emulation / torch fp32: the table of the docstring)
CAL_LV_G = 1.0                       # g, units of EPS g: 1.00 in both forms (one rounding of a quotient)
CAL_LV_SUM = 2.2                     # the summation part of the loss, units of EPS: 0.58 1.20 2.15 1.68 1.82 1.96 (the larger form)
CAL_LV_DZ_A, CAL_LV_DZ_B = 1.0, 1.35  # dz, units of EPS kf A_i: 2.78 6.74 6.69 7.65 14.92 22.26; the envelope A + B sqrt(C) =
#                                       2.91 6.88 7.19 8.76 17.53 22.56


# ---- bounds ---------------------------------------------------------------------------------------------------------------------
def g_count():
    return 1.0


def E_g():
    """relative bound of a Lovasz gradient element given the permutation"""
    return EPS * max(g_count(), CAL_LV_MARGIN * CAL_LV_G)


def sum_count(P, tile=TILE):
    rounds = min(tile // 64, -(-P // 64))
    return 2 + rounds + 6 + 1


def E_lv_loss(C, P, loss=None):
    """bound of the loss (before the scale): the probability bound (Lipschitz) plus the summation term, capped by the contract"""
    b = E_prob(C) + EPS * min(sum_count(P), CAL_LV_MARGIN * CAL_LV_SUM)
    return b if loss is None else min(b, CONTRACT_LOSS * max(1.0, abs(loss)))


def dz_count(C):
    return 3 * LB.prob_count(C) + math.log(C) + C + 6


def cal_dz(C):
    return CAL_LV_DZ_A + CAL_LV_DZ_B * math.sqrt(C)


def E_dz(C):
    """bound of a dz element in units of kf A_i"""
    return EPS * min(dz_count(C), CAL_LV_MARGIN * cal_dz(C))


# ---- float64 reference ------------------------------------------------------------------------------------------------------------
def _cp(x):
    """[N, C, H, W] -> [C, P]"""
    return np.ascontiguousarray(np.moveaxis(x, 1, 0).reshape(x.shape[1], -1))


def _ncHW(x, shape):
    """[C, P] -> [N, C, H, W]"""
    N, C, H, W = shape
    return np.ascontiguousarray(np.moveaxis(x.reshape(C, N, H, W), 0, 1))


def softmax64(z):
    zd = np.asarray(z, dtype=f64)
    e = np.exp(zd - zd.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


def closed_form_g(fgs, G):
    """fgs [C, n] bool along the sorted order, G [C] -> g [C, n] float64 (the closed form), F, I, U int64"""
    n = fgs.shape[1]
    Fc = np.cumsum(fgs, 1, dtype=np.int64)
    j = np.arange(1, n + 1, dtype=np.int64)[None]
    Gc = G.astype(np.int64)[:, None]
    I, U = Gc - Fc, Gc + (j - Fc)
    with np.errstate(divide="ignore", invalid="ignore"):
        g = np.where(fgs, 1.0 / U, I / ((U - 1).astype(f64) * U))
    g = np.where(Gc > 0, g, (j == 1).astype(f64))
    return g, Fc, I, U


def lovasz_ref(z, target, classes="present", ignore=IGNORE, perm=None, gout=1.0, gmul=1.0):
    """the definition in float64.  perm: None (the stable descending sort of the float64 errors) or int [C, nv]: pixel indices of
    the valid pixels of every class in the order to evaluate (an implementation's own permutation).
    -> dict(loss (times gmul), out3 = (loss, 1 / n, n), loss_c, g [C, P] (by pixel), m [C, P], perm, G, nv, valid, grad, kf, unit [P])"""
    assert classes in MODES
    N, C, H, W = z.shape
    p = _cp(softmax64(z))
    t = np.asarray(target).reshape(-1)
    P = t.size
    valid = t != ignore
    fg = (t[None] == np.arange(C)[:, None]) & valid[None]
    m = np.where(fg, 1.0 - p, p)
    vidx = np.flatnonzero(valid)
    nv = vidx.size
    G = fg.sum(1)
    if perm is None:
        perm = vidx[np.argsort(-m[:, vidx], axis=1, kind="stable")] if nv else np.zeros((C, 0), dtype=np.int64)
    perm = np.asarray(perm, dtype=np.int64).reshape(C, nv)
    fgs = np.take_along_axis(fg, perm, 1)
    g, _, _, _ = closed_form_g(fgs, G)
    loss_c = (np.take_along_axis(m, perm, 1) * g).sum(1)
    incl = G > 0 if classes == "present" else np.ones(C, dtype=bool)
    n = int(incl.sum())
    loss = float(loss_c[incl].sum() / n) if n else 0.0
    gpix = np.zeros((C, P))
    np.put_along_axis(gpix, perm, g, 1)
    gpix[~incl] = 0.0
    kf = float(gout) * float(gmul) / n if n else 0.0
    a = np.where(fg, -gpix, gpix) * kf
    dot = (a * p).sum(0, keepdims=True)
    grad = p * (a - dot)
    grad[:, ~valid] = 0.0
    return dict(loss=loss * float(gmul), out3=(loss, 1.0 / n if n else 0.0, n), loss_c=loss_c, g=gpix, m=m, perm=perm, G=G, nv=nv,
                valid=valid, fg=fg, grad=_ncHW(grad, z.shape), kf=kf, unit=abs(kf) * gpix.max(0), incl=incl)


def extension64(m, fg, valid, incl):
    """the Lovasz extension evaluated in float64 at given errors m [C, P] (an implementation's own fp32 errors): its value does
    not depend on how ties are ordered, so this isolates the summation error of a loss from the error of its probabilities"""
    vidx = np.flatnonzero(valid)
    if not vidx.size or not incl.any():
        return 0.0
    md = np.asarray(m, dtype=f64)[:, vidx]
    order = np.argsort(-md, axis=1, kind="stable")
    g, _, _, _ = closed_form_g(np.take_along_axis(fg[:, vidx], order, 1), fg.sum(1))
    return float((np.take_along_axis(md, order, 1) * g).sum(1)[incl].sum() / incl.sum())


def lovasz_torch64(z, target, classes="present", ignore=IGNORE, dtype=torch.float64):
    """the published way: softmax, per class torch.sort(descending, stable), cumsum, Jaccard differences, autograd.
    -> loss (float), grad [N, C, H, W] (numpy), g per included class (list of (class, perm, jaccard differences))"""
    zt = torch.from_numpy(np.ascontiguousarray(z)).to(dtype).requires_grad_(True)
    N, C, H, W = zt.shape
    probas = F.softmax(zt, 1).permute(0, 2, 3, 1).reshape(-1, C)
    labels = torch.from_numpy(np.asarray(target)).reshape(-1)
    vidx = torch.nonzero(labels != ignore)[:, 0]
    probas, labels = probas[vidx], labels[vidx]
    losses, parts = [], []
    for c in range(C):
        fgc = (labels == c).to(dtype)
        if (classes == "present" and float(fgc.sum()) == 0) or labels.numel() == 0:
            continue
        errors = (fgc - probas[:, c]).abs()
        es, perm = torch.sort(errors, dim=0, descending=True, stable=True)
        fgs = fgc[perm]
        gts = fgs.sum()
        inter = gts - fgs.cumsum(0)
        union = gts + (1 - fgs).cumsum(0)
        jac = 1.0 - inter / union
        jac = torch.cat((jac[:1], jac[1:] - jac[:-1]))
        losses.append(torch.dot(es, jac))
        parts.append((c, vidx[perm].numpy(), jac.detach().numpy()))
    if not losses:
        return 0.0, np.zeros(z.shape), parts
    loss = torch.stack(losses).mean()
    loss.backward()
    return float(loss.detach()), zt.grad.numpy(), parts


# ---- host-side restatement of the workspace and the plan -------------------------------------------------------------------------
def _up(b):
    return -(-b // ALIGN) * ALIGN


def segsort_ws_bytes(nseg, n):
    if nseg < 1 or nseg > 65535 or n < 1 or n >= 2 ** 31:
        return 0
    return _up(nseg * BINS * (-(-n // TILE)) * 4) + _up(nseg * BINS * 4)


def plan_ref(P, C, class_chunk):
    """u2pl_lovasz_plan restated -> dict with the fields of hipops.LOVASZ_PLAN_FIELDS, or None where the C side refuses"""
    if not (2 <= C <= 255 and 0 < P < 2 ** 31 and class_chunk >= 1):
        return None
    cap = min(class_chunk, C)
    tiles, nblk = -(-P // TILE), -(-P // 256)
    d = dict(chunks=-(-C // cap), cap=cap, tile=TILE, tiles=tiles, err_blocks=nblk, count_blocks=cap + 1, passes=4,
             grid_x=-(-tiles // 4), sort_scan_blocks=-(-cap * BINS // 4), grad_scan_blocks=-(-cap // 4))
    o = 0
    for name, size in (("keys", cap * P * 4), ("vals", cap * P * 4), ("keys_alt", cap * P * 4), ("vals_alt", cap * P * 4),
                       ("sort_ws", None), ("tilefg", cap * tiles * 4), ("tiletot", cap * 4), ("part", (cap + 1) * nblk * 4),
                       ("counts", (C + 1) * 4), ("slabs", C * tiles * 4)):
        d[name] = o
        o += segsort_ws_bytes(cap, P) if size is None else _up(size)
    d.pop("tiletot")
    d["total"] = o
    return d


# ---- the fp32 emulation of the kernels, and its faults ---------------------------------------------------------------------------
FAULTS = ("jaccard_diff_fp32", "unstable_ties", "ties_descending_index", "ignored_in_U", "ignored_among_m0", "absent_counted",
          "exclusive_scan", "drop_tile_carry", "drop_chunk_carry", "skip_tile_last", "bwd_no_invn")


def _exp32(x):
    return np.exp(x.astype(f64)).astype(f32)


def _butterfly(v):
    """the xor butterfly of wave_sum over the last axis (64 lanes), in v's precision; every lane ends with the same total"""
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = (v + v[..., lane ^ o]).astype(v.dtype)
    return v[..., 0]


def emu_errors(z, target, ignore=IGNORE, fault=None):
    """k_lv_errors + k_lv_counts for all classes -> keys, vals uint32 [C, P], G [C], nv, p32 [C, P], s, e"""
    N, C, H, W = z.shape
    zz = _cp(z)
    t = np.asarray(target).reshape(-1)
    P = t.size
    valid = t != ignore
    mx = zz.max(0)
    s = np.zeros(P, dtype=f32)
    for c in range(C):
        s = (s + _exp32((zz[c] - mx).astype(f32))).astype(f32)
    p = np.empty((C, P), dtype=f32)
    for c in range(C):
        p[c] = (_exp32((zz[c] - mx).astype(f32)) / s).astype(f32)
    fg = (t[None] == np.arange(C)[:, None]) & valid[None]
    m = np.where(fg, (f32(1) - p).astype(f32), p)
    keys = (np.uint32(ONE_BITS) - m.view(np.uint32)).astype(np.uint32)
    if fault == "ignored_among_m0":
        keys[:, ~valid] = np.uint32(ONE_BITS)
    elif fault != "ignored_in_U":
        keys[:, ~valid] = np.uint32(IGN_KEY)
    vals = (np.arange(P, dtype=np.uint32)[None] | (fg.astype(np.uint32) << np.uint32(31))).astype(np.uint32)
    return keys, vals, fg.sum(1).astype(np.int64), int(valid.sum()), p


def stable_sort_ref(keys, vals, bits=30):
    """numpy's stable sort of each row on the low `bits` bits of the key -> sorted keys, sorted payloads"""
    k = keys & np.uint32((1 << bits) - 1 if bits < 32 else 0xFFFFFFFF)
    order = np.argsort(k, axis=-1, kind="stable")
    return np.take_along_axis(keys, order, -1), np.take_along_axis(vals, order, -1)


def emu_sort(keys, vals, fault=None):
    if fault == "unstable_ties":                      # ties in the order of a hash of the pixel index
        tie = (vals & np.uint32(0x7FFFFFFF)).astype(np.uint64) * np.uint64(2654435761) % np.uint64(1 << 31)
    elif fault == "ties_descending_index":
        tie = np.uint64(0x7FFFFFFF) - (vals & np.uint32(0x7FFFFFFF)).astype(np.uint64)
    else:
        return stable_sort_ref(keys, vals)
    order = np.argsort((keys.astype(np.uint64) << np.uint64(32)) | tie, axis=-1, kind="stable")
    return np.take_along_axis(keys, order, -1), np.take_along_axis(vals, order, -1)


def emu_grad(skeys, svals, G, present_only, fault=None, tile=TILE):
    """k_lv_tilefg + k_ss_rowscan + k_lv_grad on sorted rows [cc, P] -> gplane rows [cc, P] f32, slabs [cc, tiles] f32, F [cc, P]"""
    cc, P = skeys.shape
    tiles = -(-P // tile)
    pad = tiles * tile - P
    valid = skeys != np.uint32(IGN_KEY)
    fg = valid & ((svals >> np.uint32(31)) != 0)
    fgp = np.pad(fg, ((0, 0), (0, pad))).reshape(cc, tiles, tile)
    tilefg = fgp.sum(2)
    carry = np.cumsum(tilefg, 1) - tilefg                       # exclusive prefix over the tiles
    if fault == "drop_tile_carry":
        carry = np.zeros_like(carry)
    inc = np.cumsum(fgp, 2)
    Fi = (carry[:, :, None] + (inc - fgp if fault == "exclusive_scan" else inc)).reshape(cc, -1)[:, :P].astype(np.int64)
    j = np.arange(1, P + 1, dtype=np.int64)[None]
    Gc = np.asarray(G, dtype=np.int64)[:, None]
    U = Gc + (j - Fi)
    with np.errstate(divide="ignore", invalid="ignore"):
        if fault == "jaccard_diff_fp32":
            J = (f32(1) - ((Gc - Fi).astype(f32) / U.astype(f32)).astype(f32)).astype(f32)
            g = np.concatenate((J[:, :1], (J[:, 1:] - J[:, :-1]).astype(f32)), 1)
        else:
            g = np.where(fg, 1.0 / U.astype(f64), (Gc - Fi).astype(f64) / ((U - 1).astype(f64) * U.astype(f64))).astype(f32)
    g = np.where(Gc > 0, g, (j == 1).astype(f32)).astype(f32)
    live = valid & ((Gc > 0) | (not present_only))
    g = np.where(live, g, f32(0)).astype(f32)
    if fault == "skip_tile_last":
        g[:, tile - 1::tile] = 0
    m = (np.uint32(ONE_BITS) - skeys).astype(np.uint32).view(f32)
    with np.errstate(invalid="ignore", over="ignore"):          # (the bits of an ignored key are no error; masked below)
        prod = np.where(live, (m * g).astype(f32), f32(0)).astype(f32)
    prod = np.pad(prod, ((0, 0), (0, pad))).reshape(cc, tiles, tile // 64, 64)
    acc = np.zeros((cc, tiles, 64), dtype=f32)
    for r in range(tile // 64):
        acc = (acc + prod[:, :, r]).astype(f32)
    slabs = _butterfly(acc)
    gplane = np.zeros((cc, P), dtype=f32)
    np.put_along_axis(gplane, (svals & np.uint32(0x7FFFFFFF)).astype(np.int64), g, 1)
    return gplane, slabs, Fi


def emu_finish(slabs, G, present_only, fault=None, cap=None):
    """k_lv_finish: lane-strided double sums of the slabs, the butterfly in double, the classes upward -> out3 (fp32)"""
    C, tiles = slabs.shape
    padded = np.pad(slabs.astype(f64), ((0, 0), (0, -(-tiles // 64) * 64 - tiles))).reshape(C, -1, 64)
    a = np.zeros((C, 64))
    for k in range(padded.shape[1]):
        a = a + padded[:, k]
    loss_c = _butterfly(a)
    total, n = 0.0, 0
    first_kept = ((C - 1) // cap) * cap if fault == "drop_chunk_carry" else 0
    for c in range(C):
        if not present_only or G[c] > 0 or fault == "absent_counted":
            if c >= first_kept:
                total += float(loss_c[c])
            n += 1
    return np.array([total / n if n else 0.0, 1.0 / n if n else 0.0, n], dtype=f32)


def emu_bwd(z, target, gplane, out3, gout=1.0, gmul=1.0, ignore=IGNORE, fault=None):
    """k_lv_bwd"""
    N, C, H, W = z.shape
    zz = _cp(z)
    t = np.asarray(target).reshape(-1)
    valid = t != ignore
    kf = f32(f32((f32(1) if fault == "bwd_no_invn" else out3[1]) * f32(gout)) * f32(gmul))
    mx = zz.max(0)
    s = np.zeros(t.size, dtype=f32)
    for c in range(C):
        s = (s + _exp32((zz[c] - mx).astype(f32))).astype(f32)
    dot = np.zeros(t.size, dtype=f32)
    sa = []
    for c in range(C):
        pr = (_exp32((zz[c] - mx).astype(f32)) / s).astype(f32)
        a = (gplane[c] * kf).astype(f32)
        a = np.where(t == c, -a, a)
        sa.append((pr, a))
        dot = (dot + (a * pr).astype(f32)).astype(f32)
    grad = np.empty((C, t.size), dtype=f32)
    for c in range(C):
        pr, a = sa[c]
        grad[c] = (pr * (a - dot).astype(f32)).astype(f32)
    grad[:, ~valid] = 0
    return _ncHW(grad, z.shape)


def emu_lovasz(z, target, classes="present", class_chunk=DEFAULT_CHUNK, gout=1.0, gmul=1.0, ignore=IGNORE, fault=None, tile=TILE):
    """all stages, chunk by chunk -> the dict lovasz_excess takes: keys, vals (stage 1), skeys, svals (stage 2), counts [C + 1],
    gplane [C, P], out3, loss, grad"""
    N, C, H, W = z.shape
    present_only = classes == "present"
    keys, vals, G, nv, _ = emu_errors(z, target, ignore, fault)
    cap = min(class_chunk, C)
    skeys, svals, gplane, slabs = np.empty_like(keys), np.empty_like(vals), [], []
    for c0 in range(0, C, cap):
        sl = slice(c0, min(c0 + cap, C))
        skeys[sl], svals[sl] = emu_sort(keys[sl], vals[sl], fault)
        gp, sb, _ = emu_grad(skeys[sl], svals[sl], G[sl], present_only, fault, tile)
        gplane.append(gp)
        slabs.append(sb)
    gplane, slabs = np.concatenate(gplane), np.concatenate(slabs)
    out3 = emu_finish(slabs, G, present_only, fault, cap)
    loss = f32(out3[0] * f32(gmul)) if gmul != 1.0 else out3[0]
    grad = emu_bwd(z, target, gplane, out3, gout, gmul, ignore, fault)
    return dict(keys=keys, vals=vals, skeys=skeys, svals=svals, counts=np.append(G, nv), gplane=gplane, out3=out3, loss=loss,
                grad=grad)


def torch_lovasz_fp32(z, target, classes="present", gout=1.0, gmul=1.0, ignore=IGNORE):
    """a torch-fp32 restatement for the calibration: F.softmax, the stable sort of its own fp32 errors, the closed form in fp32
    arithmetic on exact integer scans, torch's fp32 sum, fp32 autograd -> the dict lovasz_excess takes (no stage-1/2 fields)"""
    zt = torch.from_numpy(np.ascontiguousarray(z)).requires_grad_(True)
    N, C, H, W = zt.shape
    p = F.softmax(zt, 1).permute(1, 0, 2, 3).reshape(C, -1)
    t = torch.from_numpy(np.asarray(target)).reshape(-1)
    P = t.numel()
    valid = t != ignore
    vidx = torch.nonzero(valid)[:, 0]
    fg = (t[None] == torch.arange(C)[:, None]) & valid[None]
    m = torch.where(fg, 1 - p, p)
    G = fg.sum(1)
    incl = G > 0 if classes == "present" else torch.ones(C, dtype=torch.bool)
    n = int(incl.sum())
    gplane = torch.zeros(C, P)
    perm = vidx[torch.sort(m.detach()[:, vidx], dim=1, descending=True, stable=True).indices] if vidx.numel() else vidx[None].expand(C, 0)
    loss = zt.sum() * 0
    if vidx.numel() and n:
        fgs = torch.gather(fg, 1, perm)
        Fc = fgs.cumsum(1)
        j = torch.arange(1, vidx.numel() + 1)[None]
        I, U = G[:, None] - Fc, G[:, None] + (j - Fc)
        g = torch.where(fgs, 1 / U.float(), I.float() / ((U - 1).float() * U.float()))
        g = torch.where(G[:, None] > 0, g, (j == 1).float().expand_as(g))
        g = torch.where(incl[:, None], g, torch.zeros_like(g))
        gplane.scatter_(1, perm, g)
        loss = (torch.gather(m, 1, perm) * g).sum(1)[incl].sum() / n
    (loss * gmul).backward(torch.tensor(gout, dtype=torch.float32))
    out3 = np.array([float(loss.detach()), 1.0 / n if n else 0.0, n], dtype=f32)
    return dict(m=m.detach().numpy(), perm=perm.numpy(), gplane=gplane.numpy(), out3=out3, loss=float(loss.detach()) * gmul,
                grad=zt.grad.numpy())


# ---- the checks ------------------------------------------------------------------------------------------------------------------
def perm_of(svals, nv):
    """pixel indices of the first nv sorted payloads of every class"""
    return (np.asarray(svals)[:, :nv] & np.uint32(0x7FFFFFFF)).astype(np.int64)


def keys_excess(keys, vals, counts, z, target, ignore=IGNORE, c0=0):
    """stage 1 against float64, for the classes c0 .. c0 + rows: -> dict(m (against E_prob), fg, G, nv, behind)"""
    ref = lovasz_ref(z, target, "all", ignore)
    C = z.shape[1]
    rows = keys.shape[0]
    valid, sl = ref["valid"], slice(c0, c0 + rows)
    out = {}
    m32 = (np.uint32(ONE_BITS) - keys[:, valid]).astype(np.uint32).view(f32).astype(f64)
    out["m"] = float((np.abs(m32 - ref["m"][sl][:, valid]) / E_prob(C)).max()) if valid.any() else 0.0
    okfg = np.array_equal((vals >> np.uint32(31)).astype(bool), ref["fg"][sl])
    okpix = np.array_equal(vals & np.uint32(0x7FFFFFFF), np.broadcast_to(np.arange(valid.size, dtype=np.uint32), vals.shape))
    out["fg"] = 0.0 if okfg and okpix else math.inf
    if counts is not None:
        out["G"] = 0.0 if np.array_equal(np.asarray(counts)[sl], ref["G"][sl]) else math.inf
        out["nv"] = 0.0 if int(np.asarray(counts)[C]) == ref["nv"] else math.inf
    worst_valid = keys[:, valid].max(1, initial=0) if valid.any() else np.zeros(rows, dtype=np.uint32)
    best_ign = keys[:, ~valid].min(1, initial=0xFFFFFFFF) if (~valid).any() else np.full(rows, 0xFFFFFFFF, dtype=np.uint32)
    out["behind"] = 0.0 if bool((best_ign.astype(np.int64) > worst_valid.astype(np.int64)).all()) else math.inf
    return out


def sort_excess(keys, vals, skeys, svals, bits=30):
    rk, rv = stable_sort_ref(keys, vals, bits)
    return 0.0 if np.array_equal(rk, skeys) and np.array_equal(rv, svals) else math.inf


def lovasz_excess(got, z, target, classes="present", gout=1.0, gmul=1.0, ignore=IGNORE):
    """an implementation's outputs against the float64 definition -> dict of excesses (> 1: out of bound).  got: keys, vals,
    skeys, svals, counts (all optional: stages 1 and 2), and perm or svals, gplane [C, P], out3, loss, grad"""
    N, C, H, W = z.shape
    P = N * H * W
    ref = lovasz_ref(z, target, classes, ignore, gout=gout, gmul=gmul)
    out = {}
    if "keys" in got:
        out.update(keys_excess(got["keys"], got["vals"], got.get("counts"), z, target, ignore))
        out["sort"] = sort_excess(got["keys"], got["vals"], got["skeys"], got["svals"])
    perm = got["perm"] if "perm" in got else perm_of(got["svals"], ref["nv"])
    is_perm = all(np.array_equal(np.sort(r), np.flatnonzero(ref["valid"])) for r in perm)
    if not is_perm:
        return dict(out, perm=math.inf)
    own = lovasz_ref(z, target, classes, ignore, perm=perm, gout=gout, gmul=gmul)     # float64 under the implementation's order
    gp = np.asarray(got["gplane"], dtype=f64)
    zero = own["g"] == 0
    out["g_zero"] = 0.0 if bool((gp[zero] == 0).all()) else math.inf
    out["g"] = float((np.abs(gp - own["g"])[~zero] / (E_g() * own["g"][~zero])).max()) if (~zero).any() else 0.0
    o3 = [float(v) for v in got["out3"]]
    out["n"] = 0.0 if o3[2] == ref["out3"][2] and abs(o3[1] - ref["out3"][1]) <= EPS * ref["out3"][1] else math.inf
    b = E_lv_loss(C, P, ref["out3"][0])
    out["loss"] = max(abs(o3[0] - ref["out3"][0]) / b, abs(float(got["loss"]) - ref["loss"]) / (b * abs(gmul) + EPS * abs(ref["loss"])))
    gr = np.asarray(got["grad"], dtype=f64)
    if not np.isfinite(gr).all():
        out["dz"] = math.inf
    else:
        unit = _ncHW(np.broadcast_to(own["unit"], (C, P)).copy(), z.shape)
        live = unit > 0
        out["dz"] = float((np.abs(gr - own["grad"])[live] / (E_dz(C) * unit[live])).max()) if live.any() else 0.0
        out["dz_zero"] = 0.0 if bool((gr[~live] == 0).all()) else math.inf
    return out


# ---- the units of the calibration ---------------------------------------------------------------------------------------------
def measure_case(family, C, shape=CAL_SHAPE, form="emu", seed=0):
    """the error of one fp32 form against float64 on one logit family in the units of the CAL_LV_* constants -> dict(g, sum, dz):
    the largest over CAL_IGNORES and both class modes (scale 0.4 and an upstream gradient of 1.7 on the second)"""
    z, tgt = make_case(family, C, shape, seed)
    out = dict(g=0.0, sum=0.0, dz=0.0)
    for pat in CAL_IGNORES:
        t = apply_ignore(tgt, pat, seed)
        for mode, kw in (("present", dict()), ("all", dict(gout=1.7, gmul=0.4))):
            if form == "emu":
                got = emu_lovasz(z, t, mode, **kw)
                ref0 = lovasz_ref(z, t, mode)
                m32 = np.where(ref0["valid"][None], (np.uint32(ONE_BITS) - got["keys"]).astype(np.uint32).view(f32), f32(0))
                perm = perm_of(got["svals"], ref0["nv"])
            else:
                got = torch_lovasz_fp32(z, t, mode, **kw)
                ref0 = lovasz_ref(z, t, mode)
                m32, perm = got["m"], got["perm"]
            own = lovasz_ref(z, t, mode, perm=perm, **kw)
            nz = own["g"] > 0
            if nz.any():
                out["g"] = max(out["g"], float((np.abs(got["gplane"].astype(f64) - own["g"])[nz] / (EPS * own["g"][nz])).max()))
            out["sum"] = max(out["sum"], abs(float(got["out3"][0]) - extension64(m32, ref0["fg"], ref0["valid"], ref0["incl"])) / EPS)
            unit = _ncHW(np.broadcast_to(own["unit"], (C, tgt.size)).copy(), z.shape)
            live = unit > 0
            if live.any():
                out["dz"] = max(out["dz"], float((np.abs(got["grad"].astype(f64) - own["grad"])[live] / (EPS * unit[live])).max()))
    return out
