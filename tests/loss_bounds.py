"""Float64 references, logit families and error bounds of the per-pixel loss heads, shared by the CPU restatement
(tests/test_loss_bounds_cpu.py) and the GPU tests (tests/test_gpu_loss_bounds.py).  Not a conftest: imported by name, like bn_bounds.

Covered: u2pl_amd/csrc/losses.hip (k_ce_fwd / k_ce_finish / k_ce_bwd plain, with the unsup weight and class-weighted; k_ohem_prob,
k_ohem_apply; k_confusion) and the logit side of u2pl_amd/csrc/reliability.hip (k_bilinear_up_bwd, k_pseudo_label, k_entropy, the
k_entropy_up routes).  The references start from the fp32 inputs (a kernel's contract begins at its arguments) and are written in
torch float64, so they run on the device of their arguments; test_loss_bounds_cpu.py pins them to oracle/restate.py, to
tests/reliability_ref.py and to torch's float64 autograd.

    CE        l_i = logsumexp(z_i) - z_i[t_i];  loss = f sum_i w[t_i] l_i / D,  D = sum_i w[t_i] over the valid pixels (w = 1: n_valid),
              f = B H W / n_valid with unsup_weight (loss_helper.py:44), else 1;  out3 = {loss, f / D, D};
              grad[i, c] = (softmax_c - [c = t_i]) scale_i,  scale_i = out3[1] gout gmul w[t_i];  0 on ignored pixels
              D = 0: NaN loss, gradient 0 on ignored pixels (k_ce_finish, torch CPU), NaN on valid pixels whose weights sum to 0
    OHEM      mask_prob = softmax[t] (1.0 on ignored pixels), n_valid, threshold = +inf when min_kept > n_valid or min_kept <= 0,
              else max(float32(thresh), min(n, min_kept)-th smallest mask_prob); kept = t != ignore and mask_prob <= threshold
    pseudo    conf = max softmax = 1 / s, label = lowest index of the maximum (np.argmax on the fp32 logits: exact, no gap mask)
    entropy   -sum p log(p + 1e-10), the reference's expression; the kernels compute log s - sum e_c d_c / s without the 1e-10:
              the two differ by sum p_c log(1 + 1e-10 / p_c) <= C 1e-10, which E_ent carries as a term of its own
    bookkeeping  NaN on ignored pixels, ws[0] = n_valid, ws[128 + (f32_key(e) >> 21)]: hist0_of() of the kernel's OWN output bits
    confusion [3][C] through tests/reliability_ref.confusion_hist_t, image by image
    bilinear  ac_coord restated bit for bit; the forward is out = A_y x A_x^T with float64 matrices holding the forward's own fp32
              (i0, i1, l0, l1), the backward their transposes; the unit of its bound is |A_y|^T |g| |A_x|

THE BOUNDS come in two forms, as in contrast_bounds, and the smaller is asserted on every element:

  * a first-order rounding count read off the kernel (s_count, grad_count, loss_count, prob_count, ent_count, bil_count; one unit
    per fp32 rounding, expf / logf at 1 ulp = 2 units, the worst case of the C - 1 sequential adds of s);
  * CAL_MARGIN = 10 times a ceiling measured from THE REFERENCE'S OWN fp32 ARITHMETIC against float64 -- torch fp32
    F.cross_entropy (forward and backward), F.softmax and -(p * log(p + 1e-10)).sum(1), F.interpolate's backward -- never from a
    HIP kernel.  Measured at 2 x 23 x 31 over the five ignore patterns and the three CE forms, per family (units: a gradient element
    EPS scale; the loss EPS max(1, max|z|) f; mask_prob and conf EPS; entropy EPS max(1, ln C)):

        torch fp32     C = 2                 C = 19                C = 21                C = 33                C = 150                C = 255
                     grad loss prob  ent   grad loss prob  ent   grad loss prob  ent   grad loss prob  ent   grad  loss  prob  ent   grad  loss  prob   ent
        trained      3.48 0.22 1.42 1.41   5.75 0.10 5.70 2.22   6.57 0.36 5.77 2.30   7.21 0.48 7.02 3.74  15.32  0.24 15.31 4.70  22.73  0.22 22.71  7.06
        uniform      1.73 1.98 0.86 1.46   2.97 9.99 0.19 4.00   2.59 5.38 0.25 4.39   3.28 6.38 0.15 4.82   2.08 13.96  0.07 9.81   2.91 12.10  0.05 10.26
        saturated    3.79 0.42 1.38 1.40   3.92 1.00 2.41 0.80   5.68 1.35 2.91 0.82   4.18 0.97 2.75 0.79   4.90  0.69  3.60 0.68   5.69  1.03  3.24  0.58
        offset       2.79 0.00 1.45 1.46   6.10 0.01 4.62 2.34   6.94 0.02 5.19 2.29   6.22 0.02 5.53 3.15  15.05  0.03 14.02 4.95  19.76  0.02 19.36  5.82
        wrong        2.26 2.21 0.00 0.00   4.60 2.44 3.67 2.68   5.80 2.38 4.89 2.58   4.81 2.07 4.17 2.91   8.07  3.34  9.04 6.73   7.33  3.03  6.12  7.31
        ties         1.16 0.47 0.00 0.04   3.72 1.13 2.48 3.25   3.36 1.76 3.06 4.43   4.74 0.66 4.24 3.23   9.46  1.81  8.88 8.99  12.11  2.55 12.14 13.95
        ceiling      3.79 2.21 1.45 1.46   6.10 9.99 5.70 4.00   6.94 5.38 5.77 4.43   7.21 6.38 7.02 4.82  15.32 13.96 15.31 9.81  22.73 12.10 22.71 13.95
        emulation    3.61 1.44 1.45 1.73   6.59 4.53 5.70 1.88   7.07 3.82 5.77 2.03   7.77 4.77 7.02 2.32  16.28  6.87 15.31 6.20  23.07  6.93 22.71  9.61

    (emulation: the ceiling of the numpy fp32 emulation of the kernels' own order, for comparison; mask_prob's error is the same in
    both because the rounding of z_c - m, which both share, dominates it.)  The ceilings grow with C, so the calibrated bounds are
    functions of C -- the envelopes written beside the CAL_* constants: A + B sqrt(C) for the gradient, the probabilities and the
    entropy (an fp32 sum of C terms), 1 + ln C for the loss (its size at near-uniform logits).  Bilinear backward: 0.66 1.85 0 2.80 0
    2.31 over BIL_SHAPES (emulation 0.96 2.09 0 1.18 0 1.73).  tests/test_loss_bounds_cpu.py re-measures every figure
    (python -m pytest tests/test_loss_bounds_cpu.py -s -k ceilings) and asserts that the constants are ceilings of them.

FINDING 1: the derived count is the SMALLER bound for a gradient element and for mask_prob / conf up to C = 150 (13.1 32.3 34.4 46.9
165.4 against 38.7 77.5 80.5 95.8 181.7 calibrated units), for the loss up to C = 33 (12.2 42.7 45.3 60.0 against 44.0 102.6 105.2
116.9) and for the entropy at C = 2 only (17.1 against 17.7); above, the worst case of the C - 1 sequential adds makes the count
the larger one (270.9 against 230.8 for the gradient at C = 255, 790.6 against 148.7 for the entropy) and the calibrated bound holds
the kernels to the sqrt(C) growth that fp32 sums show.
FINDING 2: the README's "fp32 losses within 1e-4" (taken as 1e-4 max(1, |mean loss|), as contrast_bounds takes it) is the smaller
bound once max|z| reaches a few tens (saturated, offset: the unit EPS max(1, max|z|) is 6e-5 at |z| = 1000), and E_loss takes it.
It cannot hold for the unsup-weighted loss as such: the weight f = B H W / n_valid multiplies the mean and its error alike, and at
one valid pixel of 2139 the kernel's loss 1.6946547 stands 2.46e-4 from the float64 1.6944088 (1.15e-7 on the mean, 0.21 units),
the reference's own fp32 8.5e-5.  The contract is therefore applied to the mean and scaled by f.  The per-pixel loss is formed as
(m + logf(s)) - z_t, so its absolute error follows max|z| and not the loss: that is why the unit carries max(1, max|z|).
FINDING 3: the 2e-6 entropy tolerance (test_entropy_tier_b, the comment above k_entropy) is below CAL_MARGIN times the ceiling from
C = 19 on, and up to 33 classes fp32 arithmetic keeps it (ceilings 4.0 to 4.8 units = 7e-7 to 1e-6): the GPU tests assert it there
beside E_ent.  At C = 150 and 255 the reference's own fp32 expression misses it (9.81 and 13.95 units = 2.9e-6 and 4.6e-6, the
emulation 1.9e-6 and 3.2e-6): there E_ent alone is the bound.
FINDING 4 (fixed with this suite): with min_kept = 0 the reference drops nothing (loss_helper.py:519), k_sel_finish took the
smallest mask_prob as the threshold and dropped every pixel above max(that, thresh); it now returns +inf for min_kept <= 0.

The OHEM float64 rule is the one comparison that may leave pixels out: a kept target may differ from the float64 rule only inside
ohem_band(), and only the cases of ohem_rule_checked() are compared -- the `trained` family (probabilities spread over (0, 1)), a
k-th value threshold only from RULE_KTH_MIN_VALID valid pixels on (its own pixel is in the band by construction) -- for which
test_loss_bounds_cpu.py shows that the band of the float64 reference holds at most 0.1 % of the valid pixels.  Every other family
clusters its probabilities (uniform: all within 1e-3 / C of 1 / C) and is held by the exact device-rule check instead.

k_bilinear_up_bwd launches up to 2^20 blocks and takes no second grid-stride trip below 2^28 elements; no test reaches that.
No infinities or NaN in the logits, and every target in [0, C) or IGNORE: a target outside makes k_ce_fwd / k_ohem_prob read out of
bounds (the label table's job, tested elsewhere); only k_confusion, which guards them, is fed labels in [C, 255)."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from contrast_bounds import CAL_MARGIN  # noqa: F401  (one definition for all bound modules)
from reliability_ref import confusion_hist_t
from split_bounds import EPS

f32 = np.float32
IGNORE = 255
CLASSES = (2, 19, 21, 33, 150, 255)
SHAPES = ((1, 1, 1), (1, 7, 9), (3, 23, 31), (2, 65, 65))
FAMILIES = ("trained", "uniform", "saturated", "offset", "wrong", "ties")
IGNORES = ("none", "some", "image", "one", "all")
CAL_SHAPE = (2, 23, 31)          # the shape of the calibration runs
CONTRACT_LOSS = 1e-4             # README: "fp32 losses within 1e-4"
CONTRACT_ENTROPY = 2e-6          # the Tier-B entropy tolerance (test_entropy_tier_b, csrc/reliability.hip)
LOG_DELTA = 1e-10                # the reference's + 1e-10 inside the log
# the launch caps (blocks of 256 threads) above which a kernel takes a second grid-stride trip
GRID_CAPS = dict(k_ohem_prob=512, k_entropy=512, k_entropy_up=512, k_confusion=512, k_ce_fwd=2048, k_ce_bwd=4096,
                 k_pseudo_label=4096, k_bilinear_up=4096)
STRIDE_SHAPES = {512: (2, 257, 256), 2048: (2, 513, 512), 4096: (2, 725, 724)}

# ---- calibrated ceilings: the reference's own fp32 arithmetic against float64 (never the HIP kernels) ----------------------------
# Each constant is the largest value that torch's fp32 form reaches over all six families, all five ignore patterns (where a
# target exists) and C in CLASSES at 2 x 23 x 31, in the units named beside it; the asserted bound is CAL_MARGIN times that.
# Reproduce with:  python -m pytest tests/test_loss_bounds_cpu.py -s -k ceilings      (prints the table of the module docstring)
# measured ceilings at C = 2, 19, 21, 33, 150, 255 (torch fp32; the emulation of the kernels' order in brackets):
CAL_GRAD_A, CAL_GRAD_B = 2.0, 1.32  # gradient element, units of EPS scale: 3.79 6.10 6.94 7.21 15.32 22.73 [3.61 6.59 7.07 7.77
#                                     16.28 22.73]; the envelope A + B sqrt(C) = 3.87 7.75 8.05 9.58 18.17 23.08
CAL_LOSS = 2.6                      # loss, units of EPS max(1, max|z|) (1 + ln C): 2.21 9.99 5.38 6.38 13.96 12.10 [1.44 4.53 3.82
#                                     4.77 6.87 6.93] are 1.31 2.53 1.33 1.42 2.32 1.85 times (1 + ln C)
CAL_PROB_A, CAL_PROB_B = 0.5, 1.4   # mask_prob and conf, units of EPS: 1.45 5.70 5.77 7.02 15.31 22.71 [the same to two digits];
#                                     the envelope A + B sqrt(C) = 2.48 6.60 6.92 8.54 17.65 22.86
CAL_ENT_A, CAL_ENT_B = 0.5, 0.9     # entropy, units of EPS max(1, ln C): 1.46 4.00 4.43 4.82 9.81 13.95 [1.73 1.88 2.03 2.32 6.20
#                                     9.61]; the envelope A + B sqrt(C) = 1.77 4.42 4.62 5.67 11.52 14.87
CAL_BIL = 2.9                       # bilinear backward, units of EPS |A_y|^T |g| |A_x|: 0.66 1.85 0 2.80 0 2.31 over BIL_SHAPES
#                                     [0.96 2.09 0 1.18 0 1.73]


# ---- bounds ---------------------------------------------------------------------------------------------------------------------
def s_count(C):
    """relative error of s = sum_c expf(z_c - m), in units of EPS: the rounding of every d_c = z_c - m passes through e^d
    (sum p_c |d_c| <= ln C, p_c = e_c / s), expf at 1 ulp (2), the C - 1 sequential adds"""
    return (C - 1) + math.log(C) + 2


def grad_count(C):
    """first-order rounding count of a k_ce_bwd element, in units of EPS scale: the numerator expf(d) (|d| e^d <= 1/e, 1 ulp: 2),
    s (s_count), sc / s (1), e * inv (1), pr - sc (1), and the four roundings that make sc (out3[1], * gout, * gmul, * w[t])"""
    return (1 / math.e + 2) + s_count(C) + 3 + 4


def cal_grad(C):
    return CAL_GRAD_A + CAL_GRAD_B * math.sqrt(C)


def E_grad(C):
    """bound of a gradient element in units of scale = out3[1] gout gmul w[t]: derived count and calibrated bound, the smaller"""
    return EPS * min(grad_count(C), CAL_MARGIN * cal_grad(C))


def loss_count(C):
    """k_ce_fwd, per pixel, in units of EPS max(1, max|z|): the relative error of s is the absolute error of log s (s_count);
    logf at 1 ulp (2 on |log s| <= ln C); m + log s (1 on max|z| + ln C); lse - z_t (1 on |lse - z_t| <= 2 max|z| + ln C) and the
    fp32 rounding of the mean (1 on the same): C + 6 + 6 ln C.  The mean itself is accumulated in double"""
    return s_count(C) + 2 * math.log(C) + (1 + math.log(C)) + 2 * (2 + math.log(C))


def cal_loss(C):
    return CAL_LOSS * (1 + math.log(C))


def E_loss(C, zmax, factor=1.0, loss=None):
    """bound of the loss: `factor` is the unsup weight total / n_valid (1 for the plain and the class-weighted mean), which
    multiplies the mean and its error alike.  With the reference loss given, the parity contract caps the bound: 1e-4 max(1, |mean|)
    on the mean, times the same factor (FINDING 2 of the module docstring)"""
    f = abs(factor)
    b = EPS * min(loss_count(C), CAL_MARGIN * cal_loss(C)) * max(1.0, zmax) * f
    return b if loss is None else min(b, CONTRACT_LOSS * max(1.0, abs(loss) / f) * f)


def prob_count(C):
    """k_ohem_prob / k_pseudo_label: the numerator expf(z_t - m) (1/e + 2; conf's is the exact 1), s (s_count), one division; the
    value is at most 1"""
    return (1 / math.e + 2) + s_count(C) + 1


def cal_prob(C):
    return CAL_PROB_A + CAL_PROB_B * math.sqrt(C)


def E_prob(C):
    """bound of mask_prob and of conf: derived count and calibrated bound, the smaller"""
    return EPS * min(prob_count(C), CAL_MARGIN * cal_prob(C))


def ent_count(C):
    """k_entropy, in units of EPS max(1, ln C): log s carries s_count and logf's 1 ulp (2); t = sum e d: every term carries the
    rounding of d twice, expf's 2 and the product's 1 on e |d| (ln C + 4 on sum p |d| <= ln C), and the C - 1 adds; t / s: s_count
    again and the division (1); the difference (1)"""
    return 2 * s_count(C) + 2 + (math.log(C) + 4) + (C - 1) + 1 + 1


def cal_ent(C):
    return CAL_ENT_A + CAL_ENT_B * math.sqrt(C)


def E_ent(C):
    """bound of |entropy^ - (-sum p log(p + 1e-10))|: the documented difference of the two expressions, sum_c p_c log(1 + 1e-10 / p_c)
    <= C 1e-10, is part of the bound, not ignored"""
    return EPS * min(ent_count(C), CAL_MARGIN * cal_ent(C)) * max(1.0, math.log(C)) + C * LOG_DELTA


def bil_count(Ay, Ax):
    """k_bilinear_up_bwd: ky + kx products and adds of the gather (k = most outputs that read one input along an axis), the two
    weights' own sums l0 + l1, wy * racc: in units of EPS |A_y|^T |g| |A_x|"""
    return int((Ay != 0).sum(0).max()) * 2 + int((Ax != 0).sum(0).max()) * 2 + 3


def E_bil(Ay, Ax):
    return EPS * min(bil_count(Ay, Ax), CAL_MARGIN * CAL_BIL)


# ---- logit families, targets, ignore patterns ------------------------------------------------------------------------------------
def make_case(family, C, shape, seed=0):
    """-> z [N, C, H, W] float32 (finite), target [N, H, W] int64 in [0, C) from a seeded generator.
    trained: sigma 2, the target class boosted by 2 + ln C (its probability spreads over (0, 1) at every C); uniform: sigma 1e-3; saturated: sigma 40; offset: sigma 3 on +1000;
    wrong: sigma 2 with the target class at -30; ties: logits on a grid of 1/4 (natural ties), the maximum duplicated exactly in
    two classes (three on every third pixel when C >= 3), every fifth pixel constant over the classes"""
    assert family in FAMILIES
    N, H, W = shape
    rng = np.random.default_rng([seed, FAMILIES.index(family), C, N, H, W])
    t = rng.integers(0, C, (N, H, W))
    g = rng.standard_normal((N, C, H, W), dtype=f32)
    ti = t[:, None]
    if family == "trained":
        z = f32(2) * g
        np.put_along_axis(z, ti, np.take_along_axis(z, ti, 1) + f32(2 + math.log(C)), 1)
    elif family == "uniform":
        z = f32(1e-3) * g
    elif family == "saturated":
        z = f32(40) * g
    elif family == "offset":
        z = f32(3) * g + f32(1000)
    elif family == "wrong":
        z = f32(2) * g
        np.put_along_axis(z, ti, f32(-30), 1)
    else:
        z = np.round(f32(8) * g) / f32(4)
        top = z.max(1, keepdims=True) + f32(1)
        a = rng.integers(0, C, (N, 1, H, W))
        b = (a + 1 + rng.integers(0, max(C - 1, 1), (N, 1, H, W))) % C
        np.put_along_axis(z, a, top, 1)
        np.put_along_axis(z, b, top, 1)
        if C >= 3:
            c3 = (a + b + 1) % C
            third = (np.arange(N * H * W).reshape(N, 1, H, W) % 3) == 0
            np.put_along_axis(z, c3, np.where(third, top, np.take_along_axis(z, c3, 1)), 1)
        const = (np.arange(N * H * W).reshape(N, 1, H, W) % 5) == 4
        z = np.where(const, z[:, :1], z)
    z = np.ascontiguousarray(z, dtype=f32)
    assert np.isfinite(z).all()
    return z, t.astype(np.int64)


def apply_ignore(target, pattern, seed=0):
    """none | some (about 20 %) | image (one whole image of the batch; the only one when N = 1) | one (exactly one valid pixel) |
    all.  Every value stays in [0, C) or becomes IGNORE"""
    assert pattern in IGNORES
    t = target.copy()
    rng = np.random.default_rng([seed, IGNORES.index(pattern), t.size])
    if pattern == "some":
        t[rng.random(t.shape) < 0.2] = IGNORE
    elif pattern == "image":
        t[t.shape[0] // 2] = IGNORE
    elif pattern == "one":
        keep = int(rng.integers(0, t.size))
        v = t.reshape(-1)[keep]
        t[...] = IGNORE
        t.reshape(-1)[keep] = v
    elif pattern == "all":
        t[...] = IGNORE
    return t


def seeded_weights(C, seed=0):
    """a class-weight vector in (0.5, 1.5) with one exact zero"""
    rng = np.random.default_rng([seed, C, 77])
    w = rng.uniform(0.5, 1.5, C).astype(f32)
    w[int(rng.integers(0, C))] = 0.0
    return w


# ---- float64 references (torch, on the device of their arguments; they start from the fp32 inputs) ---------------------------------
def _T(x, dtype=None):
    t = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))
    return t.to(dtype) if dtype is not None else t


def softmax64(z):
    """z [N, C, H, W] float32 -> p [N, C, H, W], lse [N, H, W] in float64"""
    zd = _T(z).double()
    m = zd.amax(1, keepdim=True)
    e = (zd - m).exp()
    s = e.sum(1, keepdim=True)
    return e / s, (m + s.log())[:, 0]


def ce_ref(z, target, unsup_weight=False, class_weight=None, gout=1.0, gmul=1.0, ignore=IGNORE, sm=None):
    """F.cross_entropy(z, target, ignore_index[, weight]) [* total / n_valid] * gmul and its gradient times gout, in float64:
    loss (already times gmul), out3 = (loss before gmul, gradient scale w / den, den = n_valid or the weight sum), grad
    [N, C, H, W], scale [N, H, W] = out3[1] gout gmul w[t] (0 on ignored pixels), valid.  den = 0: NaN loss; the gradient is 0 on
    ignored pixels (k_ce_finish, torch CPU) and NaN on valid pixels whose weights sum to zero (inf * 0)"""
    z, target = _T(z), _T(target)
    p, lse = sm if sm is not None else softmax64(z)
    valid = target != ignore
    t = torch.where(valid, target, torch.zeros_like(target))
    l = lse - z.double().gather(1, t[:, None])[:, 0]
    wt = _T(class_weight).to(z.device).double()[t] if class_weight is not None else torch.ones_like(l)
    wt = wt * valid
    den = float(wt.sum())
    w = (target.numel() / den if den > 0 else math.inf) if unsup_weight else 1.0
    loss = w * float((wt * l).sum()) / den if den > 0 else math.nan
    gs = w / den if den > 0 else math.inf
    if den > 0:
        scale = wt * (gs * float(gout) * float(gmul))
    else:
        scale = torch.where(valid, torch.full_like(l, math.nan), torch.zeros_like(l))
    grad = p * scale[:, None]
    grad.scatter_add_(1, t[:, None], -scale[:, None])
    return dict(loss=loss * float(gmul), out3=(loss, gs, den), grad=grad, scale=scale, valid=valid)


def _nan_aware_excess(got, ref, bound):
    got, ref = _T(got).double(), _T(ref).double()
    if not torch.equal(torch.isnan(got), torch.isnan(ref)) or bool(torch.isinf(got).any()):
        return math.inf
    ok = ~torch.isnan(ref)
    if not bool(ok.any()):
        return 0.0
    bound = bound.double().to(got.device) if torch.is_tensor(bound) else float(bound)
    d = ((got - ref).abs() / (bound + 1e-300))[ok]
    return float(d.max())


def ce_excess(got, ref, C, zmax, gmul=1.0):
    """got: dict(loss, out3 [3], grad) of an implementation (any float type) against ce_ref's dict -> dict of excesses (> 1: out
    of bound): loss (out3[0] against E_loss with the unsup factor out3[1] out3[2]; the returned loss, times gmul, against |gmul|
    times that plus the rounding of the product), grad (every element, against E_grad(C) |scale|), gscale (out3[1]: one fp32
    rounding), count (out3[2] must be the fp32 value of n_valid / of the weight sum: 0 or inf), ignored (the gradient of an
    ignored pixel must be exactly 0)"""
    loss64, gs64, den = ref["out3"]
    o3 = [float(v) for v in got["out3"]]
    out = {}
    if math.isnan(ref["loss"]):
        out["loss"] = 0.0 if math.isnan(float(got["loss"])) and math.isnan(o3[0]) else math.inf
    else:
        b = E_loss(C, zmax, gs64 * den, loss64)
        e1 = abs(o3[0] - loss64) / b
        e2 = abs(float(got["loss"]) - ref["loss"]) / (b * abs(gmul) + EPS * abs(ref["loss"]))
        out["loss"] = max(e1, e2) if math.isfinite(o3[0]) and math.isfinite(float(got["loss"])) else math.inf
    out["count"] = 0.0 if o3[2] == float(f32(den)) else math.inf
    if math.isinf(gs64):
        out["gscale"] = 0.0 if o3[1] == gs64 else math.inf
    else:
        out["gscale"] = abs(o3[1] - gs64) / (EPS * gs64 * (1 + 1e-9))
    g = _T(got["grad"])
    out["grad"] = _nan_aware_excess(g, ref["grad"], (E_grad(C) * ref["scale"].abs())[:, None].expand_as(ref["grad"]))
    ign = ~ref["valid"]
    out["ignored"] = 0.0 if bool((g.permute(0, 2, 3, 1)[ign.to(g.device)] == 0).all()) else math.inf
    return out


def ohem_threshold(mp, n_valid, thresh, min_kept, srt=None):
    """the reference's rule (loss_helper.py:512-524) on any precision of mask_prob (all pixels, ignored ones at 1.0): +inf
    (every valid pixel kept) when min_kept > n_valid, and when min_kept <= 0 (the reference drops nothing then); else the larger
    of float32(thresh) and the min(n, min_kept)-th smallest value.  srt: the sorted values, where the caller has them"""
    if min_kept > n_valid or min_kept <= 0:
        return math.inf
    srt = torch.sort(mp.reshape(-1)).values if srt is None else srt
    return max(float(f32(thresh)), float(srt[min(srt.numel(), int(min_kept)) - 1]))


def ohem_ref(z, target, thresh, min_kept, ignore=IGNORE, sm=None):
    """-> mask_prob [N, H, W] float64 (1.0 on ignored pixels), n_valid, threshold, kept target"""
    z, target = _T(z), _T(target)
    p, _ = sm if sm is not None else softmax64(z)
    valid = target != ignore
    t = torch.where(valid, target, torch.zeros_like(target))
    mp = torch.where(valid, p.gather(1, t[:, None])[:, 0], torch.ones_like(p[:, 0]))
    nv = int(valid.sum())
    thr = ohem_threshold(mp, nv, thresh, min_kept)
    return mp, nv, thr, ohem_rule(mp, thr, target, ignore)


def ohem_rule(mp, thr, target, ignore=IGNORE):
    """kept = t != ignore and mp <= thr"""
    return torch.where((target != ignore) & (mp <= thr), target, torch.full_like(target, ignore))


def ohem_band(mp64, thr64, valid, C, thresh):
    """valid pixels whose float64 probability lies within the bound of the float64 threshold: the only pixels on which an fp32
    kept target may differ from the float64 rule.  A k-th smallest value moves by at most the largest element error, so a
    threshold that is one carries a bound of its own: 2 E_prob; the fixed float32(thresh): E_prob"""
    if math.isinf(thr64):
        return torch.zeros_like(valid)
    return valid & ((mp64 - thr64).abs() <= (2 if thr64 > float(f32(thresh)) else 1) * E_prob(C))


RULE_FAMILIES = ("trained",)               # spread probabilities: the band stays under the cap (test_loss_bounds_cpu.py)
RULE_KTH_MIN_VALID = 5000                  # a k-th value threshold has its own pixel and its neighbours in the band


def ohem_rule_checked(family, n_valid, thr64, thresh):
    """the cases of the float64-rule check"""
    kth = math.isfinite(thr64) and thr64 > float(f32(thresh))
    return family in RULE_FAMILIES and (not kth or n_valid >= RULE_KTH_MIN_VALID)


OHEM_RULE_CAP = 1e-3     # the band may hold at most 0.1 % of the valid pixels of a case


def pseudo_ref(z, sm=None):
    """-> conf [N, H, W] float64 = max softmax, label [N, H, W] int64 = lowest index of the maximum (np.argmax: exact on fp32)"""
    p, _ = sm if sm is not None else softmax64(z)
    zn = z.cpu().numpy() if torch.is_tensor(z) else z
    return p.amax(1), torch.from_numpy(zn.argmax(1).astype(np.int64))


def entropy_ref(z, sm=None):
    """the reference expression -sum p log(p + 1e-10) in float64"""
    p, _ = sm if sm is not None else softmax64(z)
    return -(p * (p + LOG_DELTA).log()).sum(1)


def f32_key(bits):
    """csrc/common.h f32_key on uint32 bit patterns"""
    bits = np.asarray(bits, dtype=np.uint32)
    return np.where(bits & np.uint32(0x80000000), ~bits, bits | np.uint32(0x80000000)).astype(np.uint32)


def hist0_of(values_f32):
    """the pass-0 histogram ws[128 + (f32_key(v) >> 21)] (2048 bins) of an array's OWN bits"""
    key = f32_key(np.ascontiguousarray(values_f32, dtype=f32).view(np.uint32).reshape(-1))
    return np.bincount((key >> np.uint32(21)).astype(np.int64), minlength=2048)


def confusion_ref(z, target, C, ignore=IGNORE):
    """[3, C] int64 through tests/reliability_ref.confusion_hist_t, image by image (its logits argument is one image)"""
    z, target = _T(z).cpu(), _T(target).cpu()
    hist = torch.zeros(3 * C, dtype=torch.int64)
    for n in range(z.shape[0]):
        confusion_hist_t(z[n], target[n], ignore, C, hist)
    return hist.reshape(3, C)


# ---- bilinear: ac_coord restated bit for bit, the forward as two matrices, the backward as their transposes ---------------------
def ac_coord(n_out, n_in):
    """csrc/common.h ac_coord for dst = 0 .. n_out - 1 -> i0, i1 (int64), l0, l1 (float32)"""
    scale = f32(n_in - 1) / f32(n_out - 1) if n_out > 1 else f32(0)
    src = (np.arange(n_out, dtype=f32) * scale).astype(f32)
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = (src - i0.astype(f32)).astype(f32)
    l0 = (f32(1) - l1).astype(f32)
    return i0, i1, l0, l1


def ac_matrix(n_out, n_in, fault=None):
    """[n_out, n_in] float64: row o holds l0 at i0 and l1 at i1 (their sum where i1 == i0).  fault "skip_i1_eq_i0": the rows whose
    two taps coincide (the last row / column, every row when n_in == 1) contribute nothing"""
    i0, i1, l0, l1 = ac_coord(n_out, n_in)
    A = np.zeros((n_out, n_in))
    o = np.arange(n_out)
    np.add.at(A, (o, i0), l0.astype(np.float64))
    np.add.at(A, (o, i1), l1.astype(np.float64))
    if fault == "skip_i1_eq_i0":
        A[i0 == i1] = 0.0
    return A


def bilinear_fwd64(x, H, W):
    x = np.asarray(x, dtype=np.float64)
    return np.einsum("oh,nchw,pw->ncop", ac_matrix(H, x.shape[2]), x, ac_matrix(W, x.shape[3]))


def bilinear_bwd64(g, h, w, fault=None):
    """the float64 transpose of the forward's own fp32 (i0, i1, l0, l1): gin [N, C, h, w], and |A_y|^T |g| |A_x| (the bound's unit)"""
    g = np.asarray(g, dtype=np.float64)
    Ay, Ax = ac_matrix(g.shape[2], h, fault), ac_matrix(g.shape[3], w, fault)
    return np.einsum("oh,ncop,pw->nchw", Ay, g, Ax), np.einsum("oh,ncop,pw->nchw", np.abs(Ay), np.abs(g), np.abs(Ax))


def bil_excess(got, g, h, w):
    ref, unit = bilinear_bwd64(g, h, w)
    Ay, Ax = ac_matrix(g.shape[2], h), ac_matrix(g.shape[3], w)
    got = np.asarray(got, dtype=np.float64)
    if not np.isfinite(got).all():
        return math.inf
    return float((np.abs(got - ref) / (E_bil(Ay, Ax) * unit + 1e-300)).max())


# ---- the reference's formulas in torch fp32 (what the calibration measures) ------------------------------------------------------
def torch_ce_fp32(z, target, unsup_weight=False, class_weight=None, gout=1.0, gmul=1.0, ignore=IGNORE):
    zt = torch.from_numpy(z).requires_grad_(True)
    tt = torch.from_numpy(target)
    w = None if class_weight is None else torch.from_numpy(np.asarray(class_weight, dtype=f32))
    raw = F.cross_entropy(zt, tt, weight=w, ignore_index=ignore)
    nv = int((tt != ignore).sum())
    den = float(nv if w is None else (w.double()[torch.where(tt != ignore, tt, 0)] * (tt != ignore)).sum())
    fac = (tt.numel() / nv if nv else math.inf) if unsup_weight else 1.0
    loss = raw * fac * gmul
    loss.backward(torch.tensor(gout, dtype=torch.float32))
    gs = fac / den if den > 0 else math.inf
    return dict(loss=loss.detach().numpy(), out3=(float(raw.detach()) * fac if den > 0 else math.nan, f32(gs), f32(den)),
                grad=zt.grad)


def torch_prob_fp32(z, target, ignore=IGNORE):
    p = F.softmax(torch.from_numpy(z), 1)
    tt = torch.from_numpy(target)
    valid = tt != ignore
    mp = torch.where(valid, p.gather(1, torch.where(valid, tt, 0)[:, None])[:, 0], torch.ones_like(p[:, 0]))
    return mp, p.amax(1)


def torch_entropy_fp32(z):
    p = F.softmax(torch.from_numpy(z), 1)
    return -(p * torch.log(p + 1e-10)).sum(1)


def torch_bilinear_bwd_fp32(g, h, w):
    x = torch.zeros(g.shape[0], g.shape[1], h, w, requires_grad=True)
    F.interpolate(x, g.shape[2:], mode="bilinear", align_corners=True).backward(torch.from_numpy(np.ascontiguousarray(g, dtype=f32)))
    return x.grad.numpy()


# ---- numpy fp32 emulations in the kernels' operation order, and their faults -------------------------------------------------------
FAULTS = ("drop_last_class", "max_over_C-1", "batch_offset_n_HW", "skip_pixel_65536", "count_ignored", "weight_at_argmax",
          "gmul_twice", "entropy_no_t_over_s", "argmax_highest_tie", "bilinear_skip_i1_eq_i0")


def _exp32(x):
    with np.errstate(over="ignore"):
        return np.exp(x.astype(np.float64)).astype(f32)


def _log32(x):
    with np.errstate(divide="ignore"):
        return np.log(x.astype(np.float64)).astype(f32)


def _rows(z, fault):
    """z [N, C, H, W] -> [N, C, HW] as the kernel addresses it: z + n C HW + q + c HW; the fault drops the C of the batch offset
    (every read stays inside the tensor)"""
    N, C, H, W = z.shape
    HW = H * W
    if fault != "batch_offset_n_HW":
        return z.reshape(N, C, HW)
    flat = z.reshape(-1)
    idx = (np.arange(N)[:, None, None] * HW + np.arange(C)[None, :, None] * HW + np.arange(HW)[None, None, :])
    return flat[idx]


def _max_sum(zz, fault):
    """m = fmaxf over the classes, s = sequential fp32 sum of expf(z_c - m)"""
    C = zz.shape[1]
    m = zz[:, :C - 1 if fault == "max_over_C-1" and C > 1 else C].max(1)
    s = np.zeros_like(m)
    for c in range(C - 1 if fault == "drop_last_class" and C > 1 else C):
        s = (s + _exp32((zz[:, c] - m).astype(f32))).astype(f32)
    return m, s


def _skipped(N, HW):
    return (np.arange(N * HW) % 65536 == 65535).reshape(N, HW)


def emu_ce(z, target, unsup_weight=False, class_weight=None, gout=1.0, gmul=1.0, ignore=IGNORE, fault=None):
    """k_ce_fwd + k_ce_finish + k_ce_bwd and the wrapper's loss * gmul: per-pixel fp32 loss m + logf(s) - z_t accumulated in
    double, out3 rounded to fp32, sc = out3[1] gout gmul [w[t]], inv = sc / s, e * inv - [c == t] sc"""
    N, C, H, W = z.shape
    HW = H * W
    zz = _rows(z, fault)
    t = target.reshape(N, HW)
    valid = t != ignore
    tt = np.where(valid, t, 0)
    m, s = _max_sum(zz, fault)
    with np.errstate(invalid="ignore", over="ignore"):      # the C - 1 maximum of the fault overflows expf
        l = ((m + _log32(s)).astype(f32) - np.take_along_axis(zz, tt[:, None], 1)[:, 0]).astype(f32)
    widx = zz.argmax(1) if fault == "weight_at_argmax" else tt
    cw = None if class_weight is None else np.asarray(class_weight, dtype=f32)
    wt = np.ones((N, HW)) if cw is None else cw[widx].astype(np.float64)
    live = valid & ~_skipped(N, HW) if fault == "skip_pixel_65536" else valid
    counted = np.ones_like(valid) if fault == "count_ignored" else live
    lsum, n = float((wt * l.astype(np.float64))[live].sum()), float(wt[counted].sum())
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        w = np.float64(N * HW) / np.float64(n) if unsup_weight else np.float64(1.0)
        out3 = np.array([w * (np.float64(lsum) / np.float64(n)), w / np.float64(n), n]).astype(f32)
        sc0 = f32(f32(out3[1] * f32(gout)) * f32(gmul))
        if fault == "gmul_twice":
            sc0 = f32(sc0 * f32(gmul))
        sc = (sc0 * cw[widx]).astype(f32) if cw is not None else np.full((N, HW), sc0, dtype=f32)
        inv = (sc / s).astype(f32)
        grad = np.empty((N, C, HW), dtype=f32)
        for c in range(C):
            pr = (_exp32((zz[:, c] - m).astype(f32)) * inv).astype(f32)
            grad[:, c] = (pr - np.where(tt == c, sc, f32(0))).astype(f32)
    grad[np.broadcast_to(~live[:, None], grad.shape)] = 0      # (a skipped pixel's gradient is never written)
    loss = f32(out3[0] * f32(gmul)) if gmul != 1.0 else out3[0]
    return dict(loss=loss, out3=out3, grad=torch.from_numpy(grad.reshape(N, C, H, W)))


def emu_ohem_prob(z, target, ignore=IGNORE, fault=None):
    """k_ohem_prob: expf(z_t - m) / s, 1.0 on ignored pixels; -> mask_prob, n_valid"""
    N, C, H, W = z.shape
    zz = _rows(z, fault)
    t = target.reshape(N, -1)
    valid = t != ignore
    m, s = _max_sum(zz, fault)
    with np.errstate(invalid="ignore", over="ignore"):
        v = (_exp32((np.take_along_axis(zz, np.where(valid, t, 0)[:, None], 1)[:, 0] - m).astype(f32)) / s).astype(f32)
    mp = np.where(valid, v, f32(1))
    live = valid
    if fault == "skip_pixel_65536":
        live = valid & ~_skipped(N, H * W)
        mp = np.where(_skipped(N, H * W), f32(0), mp)       # never written
    return mp.reshape(N, H, W), int(live.sum())


def emu_pseudo(z, fault=None):
    """k_pseudo_label: first strict maximum, 1 / s"""
    N, C, H, W = z.shape
    zz = _rows(z, fault)
    m, s = _max_sum(zz, fault)
    if fault == "argmax_highest_tie":
        lab = C - 1 - zz[:, ::-1].argmax(1)
    else:
        lab = zz[:, :C - 1 if fault == "max_over_C-1" and C > 1 else C].argmax(1)
    with np.errstate(divide="ignore", over="ignore"):
        conf = (f32(1) / s).astype(f32)
    if fault == "skip_pixel_65536":
        conf = np.where(_skipped(N, H * W), f32(0), conf)
    return conf.reshape(N, H, W), lab.reshape(N, H, W).astype(np.int64)


def emu_entropy(z, fault=None):
    """k_entropy: s += e, t += e * d class by class, logf(s) - t / s"""
    N, C, H, W = z.shape
    zz = _rows(z, fault)
    m = zz[:, :C - 1 if fault == "max_over_C-1" and C > 1 else C].max(1)
    s, t = np.zeros_like(m), np.zeros_like(m)
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(C - 1 if fault == "drop_last_class" and C > 1 else C):
            d = (zz[:, c] - m).astype(f32)
            e = _exp32(d)
            s = (s + e).astype(f32)
            t = (t + (e * d).astype(f32)).astype(f32)
        ent = _log32(s) if fault == "entropy_no_t_over_s" else (_log32(s) - (t / s).astype(f32)).astype(f32)
    if fault == "skip_pixel_65536":
        ent = np.where(_skipped(N, H * W), f32(0), ent)
    return ent.reshape(N, H, W)


def emu_bilinear_bwd(g, h, w, fault=None):
    """k_bilinear_up_bwd: per input element, rows in ascending oy, inside a row ascending ox, wy = l0 + l1 where both taps hit,
    racc += wx * g, acc += wy * racc, all fp32"""
    g = np.asarray(g, dtype=f32)
    N, C, H, W = g.shape
    taps = []
    for n_out, n_in in ((H, h), (W, w)):
        i0, i1, l0, l1 = ac_coord(n_out, n_in)
        per = []
        for i in range(n_in):
            o = np.flatnonzero((i0 == i) | (i1 == i))
            wgt = (np.where(i0[o] == i, l0[o], f32(0)) + np.where(i1[o] == i, l1[o], f32(0))).astype(f32)
            if fault == "bilinear_skip_i1_eq_i0":
                o, wgt = o[i0[o] != i1[o]], wgt[i0[o] != i1[o]]
            per.append((o, wgt))
        taps.append(per)
    out = np.zeros((N, C, h, w), dtype=f32)
    for iy, (oys, wys) in enumerate(taps[0]):
        for ix, (oxs, wxs) in enumerate(taps[1]):
            acc = np.zeros((N, C), dtype=f32)
            for oy, wy in zip(oys, wys):
                racc = np.zeros((N, C), dtype=f32)
                for ox, wx in zip(oxs, wxs):
                    racc = (racc + (wx * g[:, :, oy, ox]).astype(f32)).astype(f32)
                acc = (acc + (wy * racc).astype(f32)).astype(f32)
            out[:, :, iy, ix] = acc
    return out


# ---- the units of the calibration ---------------------------------------------------------------------------------------------
def measure_case(family, C, shape=CAL_SHAPE, form="torch", seed=0):
    """the error of one fp32 form (torch: the reference's formulas; emu: the kernels' order) against float64 on one logit
    family, in the units of the CAL_* constants -> dict(grad, loss, prob, ent): the largest over the ignore patterns and the
    three CE forms (plain, unsup weight, class weights; scale 0.4 and an upstream gradient of 1.7 on the last two)"""
    z, tgt = make_case(family, C, shape, seed)
    sm = softmax64(z)
    zmax = float(np.abs(z).max())
    out = dict(grad=0.0, loss=0.0, prob=0.0, ent=0.0)
    cw = seeded_weights(C, seed)
    for pat in IGNORES[:4]:
        t = apply_ignore(tgt, pat, seed)
        for kw in (dict(), dict(unsup_weight=True, gout=1.7, gmul=0.4), dict(class_weight=cw, gout=1.7, gmul=0.4)):
            ref = ce_ref(z, t, sm=sm, **kw)
            if not ref["out3"][2] > 0:
                continue
            got = (torch_ce_fp32 if form == "torch" else emu_ce)(z, t, **kw)
            sc = ref["scale"].abs()[:, None]
            ok = (sc > 0).expand_as(ref["grad"])
            if bool(ok.any()):
                out["grad"] = max(out["grad"], float((((_T(got["grad"]).double() - ref["grad"]).abs() / (EPS * sc + 1e-300))[ok]).max()))
            fac = abs(ref["out3"][1] * ref["out3"][2] * kw.get("gmul", 1.0))
            out["loss"] = max(out["loss"], abs(float(got["loss"]) - ref["loss"]) / (EPS * max(1.0, zmax) * fac))
        mp64 = ohem_ref(z, t, 0.7, 1, sm=sm)[0]
        mp = torch_prob_fp32(z, t)[0] if form == "torch" else _T(emu_ohem_prob(z, t)[0])
        out["prob"] = max(out["prob"], float((mp.double() - mp64).abs().max()) / EPS)
    conf = torch_prob_fp32(z, tgt)[1] if form == "torch" else _T(emu_pseudo(z)[0])
    out["prob"] = max(out["prob"], float((conf.double() - sm[0].amax(1)).abs().max()) / EPS)
    ent = torch_entropy_fp32(z) if form == "torch" else _T(emu_entropy(z))
    out["ent"] = float((ent.double() - entropy_ref(z, sm)).abs().max()) / (EPS * max(1.0, math.log(C)))
    return out


BIL_SHAPES = (((1, 1), (4, 5)), ((5, 7), (17, 23)), ((13, 16), (13, 16)), ((9, 13), (37, 52)), ((5, 7), (3, 5)), ((17, 17), (65, 65)))


def measure_bilinear(lo, hi, form="torch", seed=0, C=5):
    g = np.random.default_rng([seed, lo[0], lo[1], hi[0], hi[1]]).standard_normal((2, C, hi[0], hi[1])).astype(f32)
    ref, unit = bilinear_bwd64(g, lo[0], lo[1])
    got = torch_bilinear_bwd_fp32(g, lo[0], lo[1]) if form == "torch" else emu_bilinear_bwd(g, lo[0], lo[1])
    return float((np.abs(got.astype(np.float64) - ref) / (EPS * unit + 1e-300)).max())
