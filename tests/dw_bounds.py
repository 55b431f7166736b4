"""Shared by tests/test_dwconv_cpu.py and tests/test_gpu_dwconv.py: operands, float64 references with their bounds, the shape
list, and a numpy float32 emulation of csrc/dwconv.hip (with three deliberate faults) for the depthwise 3x3 convolution.

Oracle: torch.nn.functional.conv2d(groups=C) (and torch.nn.grad's input / weight gradients) in float64 on the CPU, on the
float32-rounded operands.  Bound of each output element:

    |got - ref| <= (n + 2) * 2^-24 * cond

cond: the same operation on absolute values (plus |bias| / |sink| where an epilogue adds one), n: the reduction length (9 taps
for y and dx, N*Ho*Wo pixels for dw).  This is the worst case of an fp32 sum of n products in any order (n roundings of partial
sums that never exceed cond, one rounding per product) plus the bias / accumulate add: derived, not fitted, the derivation of
tests/test_gpu_gconv.py.  The weight gradient's slab partial sums fit it too: a term passes through at most (pixels per thread +
lane groups + slabs) <= n additions.  Where cond is 0 (taps that only ever meet padding) the bound is 0: the result must be
exactly 0.

Channel tile of all three kernels as built: 128 channels (32 lanes x 4 channels, csrc/dwconv.hip DW_CT).  Weight-gradient slabs:
ceil(M / ns) pixels with ns = min(ceil(2048 / channel tiles), ceil(M / 64), 512), M = N*Ho*Wo."""
import numpy as np
import torch
import torch.nn.functional as F

from split_bounds import EPS, excess

# 4, 8, both sides of the tile edges at 128 and 256; 132 and 260 are no multiples of 8 above the first tile
CHANNELS = [4, 8, 124, 128, 132, 256, 260]
# (H, W, stride, dil): odd extents; stride 2; even extents at stride 2 with dilation; dilations; only the centre tap inside
GEOMS = [(13, 11, 1, 1), (9, 17, 2, 1), (12, 10, 2, 2), (13, 11, 1, 2), (9, 17, 1, 4), (9, 9, 1, 12)]
N_IMG = 2
# (N, C, H, W, stride, dil): M = 145 pixels -> 3 slabs of 49: the pixel walk crosses the first and the second slab edge inside a row
SLAB_CASE = (1, 132, 5, 29, 1, 1)
SLAB_CASE_SLABS = 3


def shape_list():
    """every (N, C, H, W, stride, dil) the GPU tests run the kernels on"""
    return [(N_IMG, C) + g for C in CHANNELS for g in GEOMS] + [SLAB_CASE]


def wgrad_slabs(M, C):
    """the slab plan of csrc/dwconv.hip (dwwgrad_plan), restated: -> (pixels per slab, slabs)"""
    tiles = -(-C // 128)
    ns = max(1, min(-(-2048 // tiles), -(-M // 64), 512))
    rows = -(-M // ns)
    return rows, -(-M // rows)


def out_size(h, stride, pad, dil):
    return (h + 2 * pad - 2 * dil - 1) // stride + 1


def operands(C, H, W, stride, dil, seed=0, N=N_IMG):
    """post-ReLU heavy-tailed x, weights N(0,1)/3, a gradient whose pixels span six decades (all float32, CPU); pad = dil"""
    g = torch.Generator().manual_seed(1000 * seed + 17 * C + H)
    pad = dil
    x = torch.relu(torch.randn(N, C, H, W, generator=g) - 0.25) ** 3
    w = torch.randn(C, 1, 3, 3, generator=g) / 3.0
    Ho, Wo = out_size(H, stride, pad, dil), out_size(W, stride, pad, dil)
    gy = torch.randn(N, C, Ho, Wo, generator=g) * 1e-4 * 10.0 ** (-6 * torch.rand(N, 1, Ho, Wo, generator=g))
    return x, w, gy, pad


def refs(x, w, gy, stride, pad, dil, bias=None, sink=None):
    """float64 {name: (ref, bound)} of y, dx, dw"""
    xd, wd, gd = x.double(), w.double(), gy.double()
    kw = dict(stride=stride, padding=pad, dilation=dil, groups=x.shape[1])
    n_px = gy.shape[0] * gy.shape[2] * gy.shape[3]

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
    return {name: (r, (n + 2) * EPS * c) for name, r, c, n in zip(("y", "dx", "dw"), ref, cond, (9, 9, n_px))}


def worst(got, ref_bounds):
    """{name: largest |got - ref| / bound} (a bound of 0 asks for an exact 0)"""
    out = {}
    for name in ("y", "dx", "dw"):
        ref, bound = ref_bounds[name]
        assert tuple(got[name].shape) == tuple(ref.shape), name
        out[name] = excess(got[name], ref, bound)
    return out


# ---- the kernels' arithmetic in numpy float32 --------------------------------------------------------------------------------
def _gather(a, hi, vh, wi, vw):
    """a[:, :, hi, wi] with zeros where a coordinate is outside (float32)"""
    g = a[:, :, np.clip(hi, 0, a.shape[2] - 1)][:, :, :, np.clip(wi, 0, a.shape[3] - 1)]
    return g * (vh[:, None] & vw[None, :]).astype(np.float32)


def emulate(x, w, gy, stride, pad, dil, fault=None):
    """y, dx, dw as csrc/dwconv.hip computes them: float32 products, float32 sums over the taps in (r, s) order, the weight
    gradient as float32 sums over pixel slabs added in slab order.  fault: None, or one deliberate mistake --
    "border": tap (2, 2) is dropped where it lands on the last row or column of the input (an off-by-one bounds test);
    "dilation": the taps are 1 apart whatever the layer's dilation; "parity": the data gradient's stride test is off by one."""
    f32 = np.float32
    x, w, gy = x.numpy().astype(f32), w.numpy().astype(f32), gy.numpy().astype(f32)
    N, C, H, W = x.shape
    Ho, Wo = gy.shape[2:]
    d = 1 if fault == "dilation" else dil
    y, dx, dw = np.zeros((N, C, Ho, Wo), f32), np.zeros((N, C, H, W), f32), np.zeros((C, 1, 3, 3), f32)
    rows, _ = wgrad_slabs(N * Ho * Wo, C)
    for r in range(3):
        for s in range(3):
            wt = w[None, :, 0, r, s, None, None]
            hi, wi = np.arange(Ho) * stride - pad + r * d, np.arange(Wo) * stride - pad + s * d
            lim_h, lim_w = (H - 1, W - 1) if (fault == "border" and r == 2 and s == 2) else (H, W)
            xg = _gather(x, hi, (hi >= 0) & (hi < lim_h), wi, (wi >= 0) & (wi < lim_w))
            y = y + xg * wt
            prod = (gy * xg).transpose(1, 0, 2, 3).reshape(C, -1)               # [C][pixels in (n, ho, wo) order]
            acc = np.zeros(C, f32)
            for s0 in range(0, prod.shape[1], rows):
                acc = acc + np.add.reduce(prod[:, s0:s0 + rows], axis=1, dtype=f32)
            dw[:, 0, r, s] = acc
            off = 1 if fault == "parity" else 0
            hh, ww = np.arange(H) + pad - r * d, np.arange(W) + pad - s * d
            ho, wo = hh // stride, ww // stride
            vh = (hh >= 0) & ((hh + off) % stride == 0) & (ho < Ho)
            vw = (ww >= 0) & ((ww + off) % stride == 0) & (wo < Wo)
            dx = dx + _gather(gy, ho, vh, wo, vw) * wt
    return dict(y=torch.from_numpy(y), dx=torch.from_numpy(dx), dw=torch.from_numpy(dw))
