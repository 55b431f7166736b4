"""Float64 reference, operand families and first-order error bounds of the contrastive kernels (u2pl_amd/csrc/contrast.hip), shared
by the CPU restatement (tests/test_contrast_bounds_cpu.py) and the GPU tests (tests/test_gpu_contrast_bounds.py).  Not a conftest:
imported by name, like bn_bounds.

One InfoNCE job (k_infonce; loss_helper.py:173-230).  f_0 is the class prototype, f_1..K the sampled rows of the class ring
(slot = head + idx, minus cap once it reaches cap), a the anchor row:

    cos_j  = (a / max(|a|, 1e-8)) . (f_j / max(|f_j|, 1e-8))
    loss_q = logsumexp_j(cos_j / temp) - cos_0 / temp
    g      = d loss_q / d a = (1 / (temp max(|a|, 1e-8))) sum_j (p_j - [j = 0]) (fhat_j - cos_j ahat)       (what `ganchor` holds)

nce_ref() is oracle.restate.info_nce's arithmetic returned per anchor and un-scaled (test_contrast_bounds_cpu.py pins the two to
each other).  temp is taken at its fp32 value: the kernel's argument is a float, its contract starts there.

THE BOUND, to first order in EPS = 2^-24, one unit per fp32 rounding, counted from k_infonce (n = D / 64 floats per lane):

  c_norm  = (n + 6) / 2 + 2        1 / max(|x|, 1e-8) by v_rsq: half the relative error of |x|^2 (an n-term FMA chain per lane and
                                   the six adds of the wave reduction -- the transposed tree for f, wave_sum_sgpr for a), plus
                                   v_rsq's 1 ulp = 2 units
  L_LOGIT = 2 (n + 6) + 8          absolute error of a logit in units of EPS / temp: c_norm (1/|a|) + 1 (ahat = a * na) + (n + 6)
                                   (the chain and tree of ahat . f, by Cauchy-Schwarz on sum |ahat_i f_i|) + c_norm (1/|f|) + 1
                                   (dot * vinv) + 1 (the division 1 / temp) + 1 (cos * inv_temp)
  X_ARG   = 6 (12 online)          the exponent's argument x = l - shift, |x| <= 2 / temp: its rounding, the rounding of x * log2(e)
                                   inside __expf and log2(e)'s own, EPS |x| each -> 3 * 2 units of EPS / temp; the online form
                                   repeats the three for the rescale factors exp(shift - mnew), whose arguments sum to <= 2 / temp
  loss    A = 2 L_LOGIT + X_ARG + 1 + 4
            sum_j |p_j - [j = 0]| <= 2 logit errors; the rounding of shift + log s (|lse| <= 1/temp + ln(K + 1)); logf at 1 ulp =
            2 units of |log s| <= 2/temp + ln(K + 1)
          B = 2 + K + 3 ln(K + 1) + 1 (+ 3 per four-row batch online)
            v_exp's 1 ulp; the K adds of the (K + 1)-term sum; the ln(K + 1) parts of the two terms above; the rounding of
            lse - l0 (relative to the loss: the bound is on |d loss_q| / max(1, |loss_q|)); online: v_exp + s *= resc per batch
          E_loss = min(EPS (A / temp + B), 1e-4)
  grad    in units of 1 / (temp max(|a|, 1e-8)), on the 2-norm of an anchor's error vector (every direction fhat_j - cos_j ahat
          has norm <= 1; the 2-norm bounds every component, so this check is the stronger one):
          A' = 2 (L_LOGIT + X_ARG)                              sum_j |d p_j| <= 2 max_j |d x_j|
          B' = (4 + K + 2 [+ 6 per batch online])               v_exp, the sum s, 1 / s
             + 2 (2 c_norm + L_LOGIT + 1) + 2 (K + 1)           fhat_j (c_norm + 1), cos_j (L_LOGIT - 2), ahat (c_norm + 1), their
                                                                product; the (K + 1)-term FMA chains of acc and of cw
             + 2 (11 + c_norm)                                  the closing expression inv_temp ((acc inv_s - f0h) - cosbar ah) na:
                                                                eleven roundings (l0 / inv_temp and inv_temp count two) and na
          E_grad = EPS (A' / temp + B')

For D = 256, K = 50: A = 67, B = 64.8, A' = 68, B' = 280.  These are worst-case counts, every rounding at full size and of one sign:
a logit alone carries L_LOGIT = 28 units, and the factor 2 of sum |p_j - [j = 0]| is attained (p_0 -> 0, one p_j -> 1: the loss is
l_j - l_0 with both logit errors at full size and opposite sign), so no rigorous count gets below 56 / temp.  fp32 arithmetic does not
behave like that, and a bound this far above it lets an error confined to one lane group or one row pass.

THE CALIBRATED BOUND is therefore asserted NEXT TO the derived one, everywhere.  It comes from the reference's own fp32 error, not
from the kernel: over all five families, temp in TEMPS and (K, D) in {(50, 256), (3, 64)} the reference's formula in fp32
(torch.cosine_similarity + F.cross_entropy) and an fp32 emulation of the kernel's order both stay below

    CAL_LOSS EPS (2 / temp + 8)   on |d loss_q| / max(1, |loss_q|)                              CAL_LOSS = 1.2
    CAL_GRAD EPS (2 / temp + 8)   on every COMPONENT of d g, in units of 1 / (temp max(|a|, 1e-8))   CAL_GRAD = 0.12

(2 / temp is the range of the exponent's argument, 8 the temp-independent roundings) and the bound is CAL_MARGIN = 10 times that:
the "about ten times" above which a bound stops counting and starts padding.  test_contrast_bounds_cpu.py re-measures both
fp32 forms against it (-s prints them): as a fraction of the calibrated bound the reference reaches 0.085 on the loss and 0.13 on a
gradient component, the emulation 0.093 and 0.10.  The bounds that the tests use:

    E_loss      = min(derived, CAL_MARGIN CAL_LOSS EPS (2 / temp + 8), 1e-4)       (the calibrated term is the smallest of the three
                                                                                     down to temp ~ 0.015, the contract below)
    E_grad      = EPS (A' / temp + B')                on the 2-norm of an anchor's error vector
    E_grad_comp = min(E_grad, CAL_MARGIN CAL_GRAD EPS (2 / temp + 8))   on every component; grad_excess() is the larger of the two ratios

FINDING: the derived E_loss exceeds the stated parity contract 1e-4 max(1, |loss|) for temp < ~0.04 (A / temp alone is 2680 units
= 1.6e-4 at 0.025) and the calibrated one for temp < ~0.015 (1.5e-4 at 0.01): there the contract is the bound (min above).
The contract of the scaled gradient, 1e-5 max(1, |g|_max), is asserted beside E_grad wherever a scaled gradient exists.

PROTOTYPES: |proto^ - proto64| <= L_proto EPS mean|x| per component.  k_proto_stream adds a wave's member rows one after the
other in fp32 (a wave owns at most ceil(P / NW) pixels, NW = 8 max(256, ceil(P / 1024)) waves), waves w and w + 4 are added (1),
the four sums pairwise (2); k_proto_finish / k_phase1_tail add the block partials in double and round the mean once (1).  Never
above n_low + 2, the bound of any order.  One dropped or doubled row moves the mean by |x| / n_low, ~1e4 units at these sizes.

Rows with 0 < |row| < 1e-8 are left out of every family: there the derivative of torch.cosine_similarity (whose clamp has a
zero sub-gradient) is neither of the two closed forms, so no reference says what the gradient should be.  Exact zero rows are in."""
import math

import numpy as np

from split_bounds import EPS, excess, recorded_calls  # noqa: F401  (re-exported: one definition for all bound modules)

CONTRACT_LOSS = 1e-4        # parity contract: |loss - ref| <= 1e-4 max(1, |loss|)
CONTRACT_GRAD = 1e-5        # ... and on the scaled gradient 1e-5 max(1, |g|_max)
TREE = 6                    # adds of a 64-lane wave reduction
NCE_FIXED_SHIFT_MAX = 80.0  # csrc/contrast.hip
CAL_LOSS = 1.2              # measured ceiling of both fp32 forms of the reference, in units of EPS (2 / temp + 8) (module docstring)
CAL_GRAD = 0.12             # ... of a gradient component, in the same units times 1 / (temp max(|a|, 1e-8))
CAL_MARGIN = 10             # a bound more than ten times what fp32 arithmetic reaches is padding
TEMPS = (0.5, 0.07, 0.025, 0.024, 0.01)
FAMILIES = ("random", "aligned", "anti", "scales", "zero")
f32 = np.float32


def temp32(temp):
    return float(f32(temp))


def is_online(temp):
    """nce_launch's choice, in its arithmetic"""
    return bool(f32(2.0) * (f32(1.0) / f32(temp)) > f32(NCE_FIXED_SHIFT_MAX))


def _counts(D, K, temp):
    n = D // 64
    online = is_online(temp)
    nbatch = (K + 1 + 3) // 4
    c_norm = (n + TREE) / 2 + 2                     # half of (n FMAs + tree), v_rsq 1 ulp
    l_logit = c_norm + 1 + (n + TREE) + c_norm + 1 + 1 + 1
    x_arg = 2 * 3 * (2 if online else 1)            # x rounding, x * log2e rounding, log2e; |x| <= 2 / temp
    return n, online, nbatch, c_norm, l_logit, x_arg


def loss_AB(D, K, temp):
    n, online, nbatch, c_norm, l_logit, x_arg = _counts(D, K, temp)
    A = 2 * l_logit + x_arg + 1 + 2 * 2             # logits, exponent arguments, shift + log s, logf on <= 2 / temp
    B = 2 + K + (1 + 2) * math.log(K + 1) + 1 + (3 * nbatch if online else 0)    # v_exp, sum, ln(K + 1) parts, lse - l0, rescales
    return A, B


def grad_AB(D, K, temp):
    n, online, nbatch, c_norm, l_logit, x_arg = _counts(D, K, temp)
    A = 2 * (l_logit + x_arg)
    B = (2 * 2 + K + 2 + (2 * 3 * nbatch if online else 0)) + 2 * (2 * c_norm + l_logit + 1) + 2 * (K + 1) + 2 * (11 + c_norm)
    return A, B


def E_loss_derived(D, K, temp):
    A, B = loss_AB(D, K, temp)
    return EPS * (A / temp32(temp) + B)


def cal_unit(temp):
    """EPS (2 / temp + 8): the range of the exponent's argument and the temp-independent roundings"""
    return EPS * (2.0 / temp32(temp) + 8.0)


def E_loss(D, K, temp):
    """bound of |loss_q^ - loss_q| / max(1, |loss_q|): derived, calibrated, contract -- the smallest"""
    return min(E_loss_derived(D, K, temp), CAL_MARGIN * CAL_LOSS * cal_unit(temp), CONTRACT_LOSS)


def E_grad(D, K, temp):
    """bound of |g^ - g|_2 temp max(|a|, 1e-8) per anchor"""
    A, B = grad_AB(D, K, temp)
    return EPS * (A / temp32(temp) + B)


def E_grad_comp(D, K, temp):
    """bound of every component of (g^ - g) temp max(|a|, 1e-8): the calibrated one (the 2-norm bound holds for a component too)"""
    return min(E_grad(D, K, temp), CAL_MARGIN * CAL_GRAD * cal_unit(temp))


def L_proto(P, n_low):
    nw = 8 * max(256, -(-P // 1024))
    return min(n_low + 2, (-(-P // nw) - 1) + 1 + 2 + 1)     # a wave's rows, w + (w + 4), the four-way combine, the mean


def proto_bound(rows64, members):
    """rows64 [P, D] float64, members: indices of the class's low-valid pixels -> per-component bound [D]"""
    return L_proto(rows64.shape[0], len(members)) * EPS * np.abs(rows64[members]).mean(0)


def loss_excess(got, ref, D, K, temp):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if not np.isfinite(got).all():
        return float("inf")
    return float((np.abs(got - ref) / (E_loss(D, K, temp) * np.maximum(1.0, np.abs(ref)))).max())


def grad_excess(got, ref, anchors, D, K, temp):
    """got / ref [..., D] un-scaled per-anchor gradients, anchors [..., D] the anchor rows"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if not np.isfinite(got).all():
        return float("inf")
    na = np.maximum(np.linalg.norm(np.asarray(anchors, dtype=np.float64), axis=-1), 1e-8)
    unit = temp32(temp) * na
    return float(max((np.linalg.norm(got - ref, axis=-1) * unit / E_grad(D, K, temp)).max(),
                     (np.abs(got - ref).max(axis=-1) * unit / E_grad_comp(D, K, temp)).max()))


# ---- float64 reference ---------------------------------------------------------------------------------------------------------
def nce_ref(anchor, feats, temp):
    """anchor [Q, D], feats [Q, 1 + K, D] (row 0: the prototype) -> loss_q [Q], g [Q, D] in float64; oracle.restate.info_nce's
    arithmetic without the mean and the 1 / Q"""
    a, f = np.asarray(anchor, dtype=np.float64), np.asarray(feats, dtype=np.float64)
    t = temp32(temp)
    na = np.maximum(np.linalg.norm(a, axis=1, keepdims=True), 1e-8)
    nf = np.maximum(np.linalg.norm(f, axis=2, keepdims=True), 1e-8)
    ah, fh = a / na, f / nf
    logit = (ah[:, None, :] * fh).sum(2) / t
    m = logit.max(1, keepdims=True)
    lse = m[:, 0] + np.log(np.exp(logit - m).sum(1))
    sm = np.exp(logit - lse[:, None])
    sm[:, 0] -= 1.0
    dah = ((sm / t)[:, :, None] * fh).sum(1)
    return lse - logit[:, 0], (dah - (dah * ah).sum(1, keepdims=True) * ah) / na


def ring_rows(ring, idx, wrap=True):
    """logical rows idx of a ring dict(storage [cap, D], cap, head): slot = head + idx, minus cap once it reaches cap.
    wrap False (the mutant): the rows behind the ring's end, as the kernel would read them -- here another ring's rows.  Those are
    unrelated rows: any bound rejects this mutant, it shows that a missing wrap is SEEN, not that the bound is tight (on the GPU the
    wrap is held by the NaN holes of the partly filled ring and by the head = cap - 2 ring)"""
    slot = ring["head"] + np.asarray(idx, dtype=np.int64)
    if wrap:
        return ring["storage"][np.where(slot >= ring["cap"], slot - ring["cap"], slot)]
    return np.concatenate([ring["storage"], ring["behind"]])[slot]


# ---- operand families ----------------------------------------------------------------------------------------------------------
# the three jobs of the kernel tests: candidate-list lengths (one of them 1), ring (cap, head, length): partly filled from 0,
# full with head = cap - 2 (most sampled rows wrap), full from 0
JOBS3 = ((1, 7, 0, 5), (5, 64, 62, 64), (11, 300, 0, 300))


def _unit(rng, shape):
    v = rng.standard_normal(shape)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _near(rng, u, n, rel=0.05):
    """n rows within rel of u (relative to |u|)"""
    return u[None, :] + rel * np.linalg.norm(u) * _unit(rng, (n, u.size)) * rng.random((n, 1))


def make_case(family, seed, D, K, Q, jobs=JOBS3, P=48):
    """-> dict: rep [P, D] f32 anchor rows; per job: cand (int32 pixel list, ascending), ia [Q], inn [Q * K] (int64 draws),
    proto [D] f32, ring dict(storage [cap, D] f32 with NaN in the unfilled slots, cap, head, length, behind).
    The last pixel of job 1's list is also on job 2's list and both jobs draw it (entry 0); in the `zero` family job 2 draws
    (entry 1) an anchor row that is exactly zero, job 1's prototype is zero and every third ring row is zero."""
    assert family in FAMILIES
    rng = np.random.default_rng([seed, FAMILIES.index(family), D, K])
    nj = len(jobs)
    rep = rng.standard_normal((P, D))
    pix = rng.permutation(P)
    cands, off = [], 0
    for j, (nc, _, _, _) in enumerate(jobs):
        c = pix[off:off + nc]
        off += nc
        if j > 0 and len(cands[j - 1]) > 1 and nc > 1:
            c = np.r_[c[:-1], cands[j - 1][-1]]          # shared with the previous job
        cands.append(np.sort(c).astype(np.int32))
    out = dict(family=family, D=D, K=K, Q=Q, P=P, jobs=[])
    dirs = _unit(rng, (nj, D)) * math.sqrt(D)
    for j, (nc, cap, head, length) in enumerate(jobs):
        u = dirs[j]
        proto = rng.standard_normal(D)
        store = rng.standard_normal((cap, D))
        if family in ("aligned", "anti"):
            sgn = 1.0 if family == "aligned" else -1.0
            proto = u.copy()
            own = [p for p in cands[j] if not (j > 0 and p in cands[j - 1])]      # a shared pixel keeps the earlier job's direction
            rep[own] = sgn * _near(rng, u, len(own))
            store = -sgn * _near(rng, u, cap)
        elif family == "scales":
            proto = proto * 10.0 ** rng.uniform(-3, 3)
            store = store * 10.0 ** rng.uniform(-3, 3, (cap, 1))
            rep[cands[j]] = rng.standard_normal((nc, D)) * 10.0 ** rng.uniform(-3, 3, (nc, 1))
        elif family == "zero":
            store[::3] = 0.0
            if j == 1 or nj == 1:
                proto = np.zeros(D)
        store = store.astype(f32)
        # logical row i lives at (head + i) % cap; the slots outside the filled range hold NaN: a read there is seen
        filled = (head + np.arange(length)) % cap
        hole = np.setdiff1d(np.arange(cap), filled)
        store[hole] = np.nan
        ia = rng.integers(0, nc, Q)
        inn = rng.integers(0, length, Q * K)
        others = np.concatenate([cands[i] for i in range(nj) if i != j] + [np.zeros(0, dtype=np.int32)])
        shared = np.intersect1d(cands[j], others)
        if shared.size:
            ia[0] = int(np.flatnonzero(cands[j] == shared[0])[0])
        out["jobs"].append(dict(cand=cands[j], ia=ia.astype(np.int64), inn=inn.astype(np.int64), proto=proto.astype(f32),
                                ring=dict(storage=store, cap=cap, head=head, length=length,
                                          behind=rng.standard_normal((cap, D)).astype(f32))))
    if family == "zero":
        jz = out["jobs"][-1]
        others = np.concatenate([c for c in cands[:-1]] + [np.zeros(0, dtype=np.int32)])
        zi = [i for i, p in enumerate(jz["cand"]) if p not in others][-1]
        rep[jz["cand"][zi]] = 0.0
        jz["ia"][Q - 1] = zi
    out["rep"] = rep.astype(f32)
    return out


def job_operands(case, j, wrap=True):
    """-> anchor pixels [Q], anchors [Q, D], feats [Q, 1 + K, D] (float32 values) of job j"""
    J, Q, K, D = case["jobs"][j], case["Q"], case["K"], case["D"]
    pix = J["cand"][J["ia"]]
    neg = ring_rows(J["ring"], J["inn"], wrap).reshape(Q, K, D)
    feats = np.concatenate([np.broadcast_to(J["proto"], (Q, 1, D)), neg], 1)
    return pix, case["rep"][pix], feats


def case_ref(case, temp):
    """float64 reference of every job: loss_q [njobs, Q], g [njobs, Q, D], anchor_pix [njobs, Q], anchors [njobs, Q, D]"""
    ls, gs, ps, an = [], [], [], []
    for j in range(len(case["jobs"])):
        pix, a, f = job_operands(case, j)
        l, g = nce_ref(a, f, temp)
        ls.append(l), gs.append(g), ps.append(pix), an.append(a)
    return np.stack(ls), np.stack(gs), np.stack(ps), np.stack(an)


def scatter_ref(case, g64, scale, gout=1.0):
    """float64 [P, D]: scale * gout * (sum of the gradients of every entry that drew the pixel)"""
    out = np.zeros((case["P"], case["D"]))
    for j, J in enumerate(case["jobs"]):
        np.add.at(out, J["cand"][J["ia"]], g64[j])
    return out * (scale * gout)


# ---- the fp32 form of the reference (torch.cosine_similarity + F.cross_entropy) ----------------------------------------------------
def torch_fp32(anchor, feats, temp):
    import torch
    import torch.nn.functional as F

    a = torch.tensor(np.asarray(anchor, dtype=f32), requires_grad=True)
    f = torch.tensor(np.asarray(feats, dtype=f32))
    logits = torch.cosine_similarity(a.unsqueeze(1), f, dim=2) / f32(temp)
    loss = F.cross_entropy(logits, torch.zeros(a.shape[0], dtype=torch.long), reduction="none")
    loss.sum().backward()
    return loss.detach().numpy(), a.grad.numpy()


# ---- fp32 emulation of k_infonce in its own order -------------------------------------------------------------------------------
MUTANTS = ("drop_row_K", "row_K_twice", "no_rescale_acc", "no_rescale_cw", "clamp_1e-8_on_square", "l0_from_row_1",
           "no_projection", "no_ring_wrap")


def _fma(a, b, c):
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(f32)


def _wave_dot(x, y, n):
    """sum_i x_i y_i over [..., D]: per lane an n-term FMA chain, then six halving adds, all in fp32"""
    xs, ys = x.reshape(x.shape[:-1] + (64, n)), y.reshape(y.shape[:-1] + (64, n))
    acc = np.zeros(xs.shape[:-1], dtype=f32)
    for i in range(n):
        acc = _fma(xs[..., i], ys[..., i], acc)
    while acc.shape[-1] > 1:
        h = acc.shape[-1] // 2
        acc = (acc[..., :h] + acc[..., h:]).astype(f32)
    return acc[..., 0]


def _rsq(x):
    return (1.0 / np.sqrt(np.asarray(x, dtype=np.float64))).astype(f32)


def _expf(x):
    """__expf: v_exp_f32 of the fp32 product x * log2(e)"""
    return np.exp2((np.asarray(x, dtype=f32) * f32(1.4426950408889634)).astype(f32).astype(np.float64)).astype(f32)


def emulate_job(anchor, feats, temp, mutant=None):
    """anchor [Q, D], feats [Q, 1 + K, D] float32 -> loss_q [Q], g [Q, D] float32 as k_infonce computes them"""
    a_all, f_all = np.asarray(anchor, dtype=f32), np.asarray(feats, dtype=f32)
    Q, D = a_all.shape
    K = f_all.shape[1] - 1
    n = D // 64
    inv_temp = f32(1.0) / f32(temp)
    online = is_online(temp)
    clamp = f32(1e-8) if mutant == "clamp_1e-8_on_square" else f32(1e-16)
    loss, grad = np.empty(Q, dtype=f32), np.empty((Q, D), dtype=f32)
    for q in range(Q):
        a, f = a_all[q], f_all[q]
        na = _rsq(np.maximum(_wave_dot(a, a, n), clamp))
        ah = (a * na).astype(f32)
        vn, vd = _wave_dot(f, f, n), _wave_dot(np.broadcast_to(ah, f.shape), f, n)
        vinv = _rsq(np.maximum(vn, clamp))
        vcos = (vd * vinv).astype(f32)
        vl = (vcos * inv_temp).astype(f32)
        s, cw, acc = f32(0), f32(0), np.zeros(D, dtype=f32)
        shift = f32(-np.inf) if online else inv_temp
        l0 = vl[1] if mutant == "l0_from_row_1" else vl[0]
        for j0 in range(0, K + 1, 4):
            rows = np.minimum(np.arange(j0, j0 + 4), K)
            if online:
                mnew = max(shift, vl[rows].max())
                resc = _expf(f32(shift - mnew)) if np.isfinite(shift) else f32(0)
                shift = mnew
                s = f32(s * resc)
                if mutant != "no_rescale_cw":
                    cw = f32(cw * resc)
                if mutant != "no_rescale_acc":
                    acc = (acc * resc).astype(f32)
            w4 = _expf((vl[rows] - shift).astype(f32))
            wn4 = (w4 * vinv[rows]).astype(f32)
            for u in range(4):
                j = j0 + u
                if j > K and mutant != "row_K_twice":
                    continue
                if j >= K and mutant == "drop_row_K":
                    continue
                s = f32(s + w4[u])
                cw = _fma(w4[u], vcos[rows[u]], cw)
                acc = _fma(wn4[u], f[rows[u]], acc)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            lse = f32(shift + f32(np.log(np.float64(s))))
            loss[q] = f32(lse - l0)
            inv_s = f32(1.0) / s
            cosbar = f32(f32(cw * inv_s) - f32(l0 / inv_temp))
            f0h = (f[0] * vinv[0]).astype(f32)
            proj = (cosbar * ah).astype(f32) if mutant != "no_projection" else np.zeros(D, dtype=f32)
            grad[q] = ((inv_temp * (((acc * inv_s).astype(f32) - f0h).astype(f32) - proj).astype(f32)).astype(f32) * na).astype(f32)
    return loss, grad


def emulate_case(case, temp, mutant=None):
    ls, gs = [], []
    for j in range(len(case["jobs"])):
        _, a, f = job_operands(case, j, wrap=mutant != "no_ring_wrap")
        l, g = emulate_job(a, f, temp, mutant)
        ls.append(l), gs.append(g)
    return np.stack(ls), np.stack(gs)


# ---- the job table and buffers of a case on the device (modelled on hipops.infonce_loss) -----------------------------------------
def device_case(case, dev, ld=None, rows_past_Q=0, sentinel=-7.0):
    """-> dict of device tensors: rep (a [P, D] column slice of a [P, ld] buffer when ld > D), jobs [njobs, 7] int64 (56-byte
    records: cand, idx_a, idx_n, proto, ring base, cap, head), groups [3, njobs * Q] (order, seg_pos, seg_len), the outputs
    loss_q / ganchor / apix / nxt (with rows_past_Q extra rows per buffer, pre-filled with the sentinel) and head [P] = -1;
    `keep` holds what the job records point to."""
    import torch
    from u2pl_amd import hipops as H

    D, K, Q, P, nj = case["D"], case["K"], case["Q"], case["P"], len(case["jobs"])
    ld = ld or D
    buf = torch.full((P, ld), float("nan"), dtype=torch.float32, device=dev)
    c0 = (ld - D) // 2 // 4 * 4
    rep = buf[:, c0:c0 + D]
    rep.copy_(torch.from_numpy(case["rep"]))
    keep, jb = [buf], np.zeros((nj, 7), dtype=np.int64)
    for j, J in enumerate(case["jobs"]):
        t = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (J["cand"], J["ia"], J["inn"], J["proto"], J["ring"]["storage"])]
        keep += t
        jb[j] = [x.data_ptr() for x in t] + [J["ring"]["cap"], J["ring"]["head"]]
    n = nj * Q + rows_past_Q
    return dict(rep=rep, ld=ld, jobs=torch.from_numpy(jb).to(dev), keep=keep,
                groups=torch.from_numpy(H.group_entries([J["ia"] for J in case["jobs"]], Q)).to(dev),
                loss_q=torch.full((n,), sentinel, dtype=torch.float32, device=dev),
                ganchor=torch.full((n, D), sentinel, dtype=torch.float32, device=dev),
                apix=torch.full((n,), int(sentinel), dtype=torch.int32, device=dev),
                nxt=torch.full((n,), int(sentinel), dtype=torch.int32, device=dev),
                head=torch.full((P,), -1, dtype=torch.int32, device=dev))
