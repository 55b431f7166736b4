"""Element-wise float64 error bounds of the split-fp16 products, shared by the CPU restatement
(tests/test_split_fp32_cpu.py) and the GPU route tests (tests/test_gpu_split_bounds.py).  Not a conftest: imported by name.

For a product C = A * B (a GEMM, or a convolution read as one) the bound of each output is

    |got - ref| <= A_REL * 2^-24 * (|A| * |B|)
                 + B_FLOOR * 2^-40 * (max|A| * (1 * |B|) + max|B| * (|A| * 1))
                 + the fp32 roundings of an epilogue (bias, eval BatchNorm, residual / GradJoin running sum, accumulate = 1)

where `*` is the same product run on absolute values or on all-ones operands.  How the constants follow from section 4:

  * Representation.  x s (s = 2^e, max|x s| in [2^14, 2^15)) is carried as h0 + h1 to within 2^-23 |x s| while both pieces are
    normal fp16; a subnormal piece adds at most half the fp16 subnormal spacing, 2^-25, i.e. 2^-25 / s <= 2^-39 max|X| (the
    maximum can sit at the bottom of [2^14, 2^15): the documented "2^-40 of the maximum" is the top of that interval).  The dropped
    a1 b1 is <= 2^-22 |ab|.  Per product: 2^-23 + 2^-23 + 2^-22 = 8 units of 2^-24 |a||b|, plus 2^-39 (max|A| |b| + max|B| |a|).
  * B_FLOOR = 4 = 2 (the 2^-39 above, in units of 2^-40) x 2 (headroom for the second-order terms: floor x floor and the subnormal
    parts of a1 b1, each below 2^-10 of the first-order floor).
  * A_REL = 64 is a TYPICAL-CASE CAP, not a derived worst case: the 8 representation units above plus 56 units for the fp32
    accumulation of the n = 3 ceil(K/16) matrix-core updates.  The worst case of an fp32 sum of n terms is n roundings of the
    largest partial sum (216 units for K = 1152, 3456 for the ASPP's K = 18432); its typical size is sqrt(n) (15 and 59).  The
    issue that introduced this bound caps the relative part at the 64 units the suite has held every split arithmetic to since
    round 3 (test_split_fp32_products_on_adversarial_operands), so a kernel that loses precision in its accumulation by more than
    the typical sqrt(n) growth fails here even where a worst-case bound would still let it pass.
  * Winograd layers: the same terms formed in the transform domain (operands B^T d B and G g G^T, whose conditions are
    |B^T| |d| |B| and |G| |g| |G^T|), pushed through |A^T| . |A|, plus C_XFORM units per fp32 transform (input, filter, output;
    each is two passes of at most 4 roundings, and the constants 1/6, 1/12, 1/24 of G are themselves rounded: 12 units).

None of the constants is fitted to a measured error: tests/test_split_fp32_cpu.py shows that the bound rejects emulations with
flushed subnormals, a mis-placed scale, a dropped piece product or a maximum below the true one (on the six-decade gradient rows:
there the floor is small against the outputs).  Where operands span twelve decades the floor term max|A| (1 * |B|) is LARGER
than the O(1) outputs, so on such data the bound only catches gross failures (non-finite values, a maximum below the truth);
the data that keep the floor small are what hold a kernel to fp32 accuracy."""
import contextlib

import numpy as np
import torch
import torch.nn.functional as F

EPS = 2.0 ** -24
A_REL = 64.0
B_FLOOR = 4.0
FLOOR = B_FLOOR * 2.0 ** -40
C_XFORM = 12.0
C_EPI = 4.0       # fp32 roundings of an epilogue: (v - mean) * invstd * gamma + beta + res (and the device's own invstd)


@contextlib.contextmanager
def recorded_calls(nn_mod):
    """record the C-ABI calls u2pl_amd.nn makes while the block runs: name -> list of argument tuples (proves a route ran)"""
    seen = {}
    real = nn_mod.call

    def rec(name, *args):
        seen.setdefault(name, []).append(args)
        return real(name, *args)
    nn_mod.call = rec
    try:
        yield seen
    finally:
        nn_mod.call = real


# ---- plain GEMM / convolution forms -----------------------------------------------------------------------------------------
def gemm_bound(A, B, a_max=None, b_max=None):
    """A [M, K], B [K, N] float64 (numpy) -> per-output bound [M, N]"""
    aa, ba = np.abs(A), np.abs(B)
    a_max = aa.max() if a_max is None else a_max
    b_max = ba.max() if b_max is None else b_max
    return A_REL * EPS * (aa @ ba) + FLOOR * (a_max * (np.ones_like(A) @ ba) + b_max * (aa @ np.ones_like(B)))


def _conv3(x, w, gy, stride, pad, dil):
    xx, ww = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = F.conv2d(xx, ww, stride=stride, padding=pad, dilation=dil)
    y.backward(gy)
    return y.detach(), xx.grad, ww.grad


def conv_refs(x, w, gy, stride=1, pad=0, dil=1):
    """float64 y = conv(x, w), dx, dw (for the incoming gradient gy) and each one's bound: dict name -> (ref, bound).
    The operands of y are (x, w), of dx (gy, w), of dw (gy, x); each is split with its own tensor maximum."""
    x, w, gy = (t.detach().cpu().double() for t in (x, w, gy))
    xa, wa, ga = x.abs(), w.abs(), gy.abs()
    mx, mw, mg = float(xa.max()), float(wa.max()), float(ga.max())
    one_x, one_w, one_g = torch.ones_like(x), torch.ones_like(w), torch.ones_like(gy)
    ref = _conv3(x, w, gy, stride, pad, dil)
    cond = _conv3(xa, wa, ga, stride, pad, dil)
    p1 = _conv3(one_x, wa, one_g, stride, pad, dil)     # y: 1 * |w|     dx: 1 * |w|
    p2 = _conv3(xa, one_w, ga, stride, pad, dil)        # y: |x| * 1     dx: |gy| * 1
    p3 = _conv3(xa, wa, one_g, stride, pad, dil)        # dw: 1 (gy) with |x|
    p4 = _conv3(one_x, wa, ga, stride, pad, dil)        # dw: |gy| with 1 (x)
    out = {}
    out["y"] = (ref[0], A_REL * EPS * cond[0] + FLOOR * (mx * p1[0] + mw * p2[0]))
    out["dx"] = (ref[1], A_REL * EPS * cond[1] + FLOOR * (mg * p1[1] + mw * p2[1]))
    out["dw"] = (ref[2], A_REL * EPS * cond[2] + FLOOR * (mg * p3[2] + mx * p4[2]))
    return out


def conv_y_bound(x, w, stride=1, pad=0, dil=1):
    """the forward alone (operands x, w): (ref, bound) -- three float64 convolutions instead of conv_refs' fifteen"""
    x, w = x.detach().cpu().double(), w.detach().cpu().double()
    xa, wa = x.abs(), w.abs()
    c = lambda a, b: F.conv2d(a, b, stride=stride, padding=pad, dilation=dil)     # noqa: E731
    return c(x, w), A_REL * EPS * c(xa, wa) + FLOOR * (float(xa.max()) * c(torch.ones_like(x), wa) + float(wa.max()) * c(xa, torch.ones_like(w)))


def conv_dx_bound(gy, w, in_hw, stride=1, pad=0, dil=1):
    """the data gradient alone (operands gy, w; input map in_hw): (ref, bound)"""
    gy, w = gy.detach().cpu().double(), w.detach().cpu().double()
    ga, wa = gy.abs(), w.abs()
    shape = (gy.shape[0], w.shape[1]) + tuple(in_hw)

    def c(g_, w_):
        return torch.nn.grad.conv2d_input(shape, w_, g_, stride=stride, padding=pad, dilation=dil)
    return c(gy, w), A_REL * EPS * c(ga, wa) + FLOOR * (float(ga.max()) * c(torch.ones_like(gy), wa) + float(wa.max()) * c(ga, torch.ones_like(w)))


def conv_dw_bound(gy, x, ksize, stride=1, pad=0, dil=1):
    """the weight gradient alone (operands gy, x; filter ksize = (R, S)): (ref, bound)"""
    gy, x = gy.detach().cpu().double(), x.detach().cpu().double()
    ga, xa = gy.abs(), x.abs()
    shape = (gy.shape[1], x.shape[1]) + tuple(ksize)

    def c(g_, x_):
        return torch.nn.grad.conv2d_weight(x_, shape, g_, stride=stride, padding=pad, dilation=dil)
    return c(gy, x), A_REL * EPS * c(ga, xa) + FLOOR * (float(ga.max()) * c(torch.ones_like(gy), xa) + float(xa.max()) * c(ga, torch.ones_like(x)))


def self_relative_fraction(got, ref, thresh=2.0 ** -16):
    """fraction of the non-zero reference outputs whose error relative to themselves exceeds thresh"""
    got = got.detach().cpu().double()
    nz = ref != 0
    if not bool(nz.any()):
        return 0.0
    return float((((got - ref).abs() > thresh * ref.abs()) & nz).sum() / nz.sum())


def excess(got, ref, bound):
    """largest |got - ref| / bound (> 1: the bound is violated; inf: a non-finite output)"""
    got = got.detach().cpu().double() if torch.is_tensor(got) else torch.as_tensor(np.asarray(got, dtype=np.float64))
    ref = ref if torch.is_tensor(ref) else torch.as_tensor(ref)
    bound = bound if torch.is_tensor(bound) else torch.as_tensor(bound)
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    return float(((got - ref).abs() / (bound + 1e-300)).max())


# ---- Winograd F(2x2, 3x3) / F(4x4, 3x3), restated from u2pl_amd/csrc/wino.hip ---------------------------------------------
def wino_mats(mt):
    """B^T [a][a], G [a][3], A^T [mt][a] in float64 (WinoT<mt>::bt / gg / at)"""
    if mt == 4:
        BT = [[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0],
              [0, 4, 0, -5, 0, 1]]
        G = [[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6],
             [0, 0, 1]]
        AT = [[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]]
    elif mt == 2:
        BT = [[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]]
        G = [[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]]
        AT = [[1, 1, 1, 0], [0, 1, -1, -1]]
    else:
        raise ValueError(mt)
    return tuple(torch.tensor(m, dtype=torch.float64) for m in (BT, G, AT))


def _tiles(x, dil, mt):
    """x [N][C][H][W] -> input tiles [N][C][T][a][a] of the padded polyphase sub-images (T = dil * dil * Ty * Tx, tile order
    (py, px, ty, tx) as in wino.hip), plus the geometry needed to put output tiles back"""
    N, C, H, W = x.shape
    a = mt + 2
    Hs, Ws = -(-H // dil), -(-W // dil)
    Ty, Tx = -(-Hs // mt), -(-Ws // mt)
    out = []
    for py in range(dil):
        for px in range(dil):
            sub = x[:, :, py::dil, px::dil]
            p = torch.zeros(N, C, Ty * mt + 2, Tx * mt + 2, dtype=x.dtype)
            p[:, :, 1:1 + sub.shape[2], 1:1 + sub.shape[3]] = sub
            t = p.unfold(2, a, mt).unfold(3, a, mt)                  # [N][C][Ty][Tx][a][a]
            out.append(t.reshape(N, C, Ty * Tx, a, a))
    return torch.cat(out, 2), (N, H, W, dil, mt, Ty, Tx)


def _untile(Y, geo):
    """output tiles [N][O][T][mt][mt] -> [N][O][H][W]"""
    N, H, W, dil, mt, Ty, Tx = geo
    O = Y.shape[1]
    out = torch.zeros(N, O, H, W, dtype=Y.dtype)
    Y = Y.reshape(N, O, dil, dil, Ty, Tx, mt, mt)
    for py in range(dil):
        for px in range(dil):
            s = Y[:, :, py, px].permute(0, 1, 2, 4, 3, 5).reshape(N, O, Ty * mt, Tx * mt)
            h, w = out[:, :, py::dil, px::dil].shape[2:]
            out[:, :, py::dil, px::dil] = s[:, :, :h, :w]
    return out


def _out_tiles(y, dil, mt):
    """[N][O][H][W] -> output-side tiles [N][O][T][mt][mt] (zero beyond the map): the gradient's tiles"""
    N, O, H, W = y.shape
    Hs, Ws = -(-H // dil), -(-W // dil)
    Ty, Tx = -(-Hs // mt), -(-Ws // mt)
    out = []
    for py in range(dil):
        for px in range(dil):
            sub = y[:, :, py::dil, px::dil]
            p = torch.zeros(N, O, Ty * mt, Tx * mt, dtype=y.dtype)
            p[:, :, :sub.shape[2], :sub.shape[3]] = sub
            out.append(p.reshape(N, O, Ty, mt, Tx, mt).permute(0, 1, 2, 4, 3, 5).reshape(N, O, Ty * Tx, mt, mt))
    return torch.cat(out, 2)


def _lr(L, t, R):
    return L @ t @ R


def wino_conv(x, w, dil, mt, with_bound=True):
    """stride-1 'same' 3x3 convolution (padding = dilation = dil) in Winograd form, float64: -> y (and its bound).
    The data gradient of such a layer is wino_conv(gy, w.flip(2, 3).transpose(0, 1), dil, mt)."""
    BT, G, AT = wino_mats(mt)
    x, w = x.detach().cpu().double(), w.detach().cpu().double()
    d, geo = _tiles(x, dil, mt)
    V = _lr(BT, d, BT.T)                                            # [N][C][T][a][a]
    U = _lr(G, w, G.T)                                              # [O][C][a][a]
    M = torch.einsum("ocij,nctij->notij", U, V)
    y = _untile(_lr(AT, M, AT.T), geo)
    if not with_bound:
        return y
    BTa, Ga, ATa = BT.abs(), G.abs(), AT.abs()
    Va, Ua = _lr(BTa, d.abs(), BTa.T), _lr(Ga, w.abs(), Ga.T)
    u_max = U.abs().amax(dim=(0, 1))                                # per component: the weight planes' per-matrix maxima
    E = ((A_REL + 2 * C_XFORM) * EPS * torch.einsum("ocij,nctij->notij", Ua, Va)
         + FLOOR * (float(V.abs().max()) * torch.einsum("ocij,nctij->notij", U.abs(), torch.ones_like(V))
                    + u_max * torch.einsum("ocij,nctij->notij", torch.ones_like(U), V.abs())))
    bound = _untile(_lr(ATa, E, ATa.T) + C_XFORM * EPS * _lr(ATa, torch.einsum("ocij,nctij->notij", Ua, Va), ATa.T), geo)
    return y, bound


def wino_wgrad(x, gy, dil, mt, nsplit=1, with_bound=True):
    """Winograd-domain weight gradient of that layer: dU = sum_tiles (A dY A^T) (x) (B^T x B), dW = G^T dU G (float64), and its
    bound (nsplit: partial sums of the tile reduction added in fp32 by the finish kernel)"""
    BT, G, AT = wino_mats(mt)
    x, gy = x.detach().cpu().double(), gy.detach().cpu().double()
    d, _ = _tiles(x, dil, mt)
    g = _out_tiles(gy, dil, mt)
    V = _lr(BT, d, BT.T)                                            # [N][C][T][a][a]
    Mg = _lr(AT.T, g, AT)                                           # [N][O][T][a][a]
    dU = torch.einsum("notij,nctij->ocij", Mg, V)
    dw = _lr(G.T, dU, G)
    if not with_bound:
        return dw
    BTa, Ga, ATa = BT.abs(), G.abs(), AT.abs()
    Va, Ma = _lr(BTa, d.abs(), BTa.T), _lr(ATa.T, g.abs(), ATa)
    condU = torch.einsum("notij,nctij->ocij", Ma, Va)
    E = ((A_REL + 2 * C_XFORM) * EPS * condU
         + FLOOR * (float(Mg.abs().max()) * torch.einsum("notij,nctij->ocij", torch.ones_like(Mg), V.abs())
                    + float(V.abs().max()) * torch.einsum("notij,nctij->ocij", Mg.abs(), torch.ones_like(V))))
    bound = _lr(Ga.T, E, Ga) + (C_XFORM + nsplit) * EPS * _lr(Ga.T, condU, Ga)
    return dw, bound


# ---- the split-fp16 GEMM, emulated (u2pl_amd/csrc/conv_geom.h) -------------------------------------
def split2_exp(amax):
    """the kernels' scale exponent: amax * 2^e lies in [2^14, 2^15) (split2_exp_bits: from the exponent field of max |x|)"""
    ex = int((np.float32(amax).view(np.uint32) >> 23) & 0xFF)
    return min(14 - (ex - 127), 126)


def _f16(v, flush):
    with np.errstate(over="ignore"):
        h = v.astype(np.float16)
    if flush:
        h = np.where(np.abs(h) < np.float16(2.0 ** -14), np.float16(0), h)
    return h


def split2(x, e, flush=False):
    """-> (h0, h1) of x * 2^e, fp16 with subnormals (flush=True: subnormals flushed to zero)"""
    with np.errstate(over="ignore", invalid="ignore"):
        xs = (np.asarray(x, dtype=np.float32) * np.float32(2.0) ** e).astype(np.float32)
        h0 = _f16(xs, flush)
        h1 = _f16((xs - h0.astype(np.float32)).astype(np.float32), flush)
    return h0, h1


def emulate_gemm(A, B, a_amax=None, b_amax=None, flush=False, e_shift=0, swap_scales=False, drop=None):
    """A [M, K] @ B [K, N] in the split-fp16 arithmetic: per-tensor power-of-two scales from the maxima, two fp16 pieces per
    operand, a1 b0 + a0 b1 + a0 b0 per 16-deep block into an fp32 accumulator, scaled back by 2^-(ea + eb).
    The keyword arguments make the mutants the bound must reject: flush (fp16 subnormals flushed), e_shift (scale exponent off by
    this much), swap_scales (each operand scaled by the OTHER one's exponent), drop (index 0..2 of a piece product left out),
    a_amax / b_amax (the maximum handed to the kernel; default the true one)."""
    A, B = np.asarray(A, dtype=np.float32), np.asarray(B, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        ea = split2_exp(np.abs(A).max() if a_amax is None else a_amax) + e_shift
        eb = split2_exp(np.abs(B).max() if b_amax is None else b_amax) + e_shift
    if swap_scales:
        ea, eb = eb, ea
    a0, a1 = (p.astype(np.float64) for p in split2(A, ea, flush))
    b0, b1 = (p.astype(np.float64) for p in split2(B, eb, flush))
    terms = [(a1, b0), (a0, b1), (a0, b0)]
    if drop is not None:
        del terms[drop]
    acc = np.zeros((A.shape[0], B.shape[1]), dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for k0 in range(0, A.shape[1], 16):
            for pa, pb in terms:
                acc = (acc.astype(np.float64) + pa[:, k0:k0 + 16] @ pb[k0:k0 + 16]).astype(np.float32)
        return np.ldexp(acc.astype(np.float64), -(ea + eb))


def operands(kind, M, K, N, seed=0):
    """float32 GEMM operands A [M, K], B [K, N] of the kinds the GPU tests use"""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((M, K))
    B = rng.standard_normal((K, N)) / np.sqrt(K)
    if kind == "relu_heavy_tail":            # post-ReLU: 60 % zeros, the rest |N(0,1)|^3
        A = np.maximum(A - 0.25, 0) ** 3
    elif kind == "six_decade_rows":          # B^T is a gradient whose rows (pixels) span six decades: A = dY [pixels][Cout]
        A = A * 1e-4 * 10.0 ** (-6 * rng.random((M, 1)))
    elif kind == "twelve_decade_channels":   # reduction channels scaled 10^U(-6, 6), the weights by the inverse
        sc = 10.0 ** (rng.random(K) * 12 - 6)
        A, B = A * sc, B / sc[:, None]
    elif kind == "cancellation":             # +w, -w on neighbouring channels with nearly equal activations
        base = rng.standard_normal((M, K // 2))
        A = np.stack((base, base * (1 + 1e-4 * rng.standard_normal(base.shape))), 2).reshape(M, K)
        bh = rng.standard_normal((K // 2, N)) / np.sqrt(K)
        B = np.stack((bh, -bh), 1).reshape(K, N)
    else:
        raise ValueError(kind)
    return A.astype(np.float32), B.astype(np.float32)


KINDS = ("relu_heavy_tail", "six_decade_rows", "twelve_decade_channels", "cancellation")
