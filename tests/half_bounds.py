"""Element-wise float64 error bound of one fused fp16 layer (csrc/half.hip: u2pl_hconv2d_fwd_f16 / u2pl_hconv2d_stem_f16),
its float64 reference, and a numpy emulation of the layer with switchable faults.  Imported by name, like split_bounds.py.

On fp16-representable operands (so there is no representation term: fp16 x fp16 products are exact in fp32)

    |got - ref64| <= 2^-11 |ref64| + 2^-25  +  A 2^-24 (|x| (*) |w|) |scale|  +  C_EPI 2^-24 (|acc scale| + |shift| + |res|)

  2^-11 |ref64| + 2^-25   the single output rounding: half an fp16 ulp, and half the subnormal spacing 2^-24
  A = 56                  the fp32 accumulation allowance split_bounds.py documents (A_REL = 64 there covers accumulation AND the
                          operand split's 8 representation units; without a split 56 remain), times the absolute-value
                          convolution: every partial sum is bounded by it
  C_EPI = 4               the epilogue's fp32 roundings (scale, shift, residual), from split_bounds.py
For fp32 output the first two terms are dropped.  Nothing here is fitted to a measured error.
"""
import numpy as np
import torch
import torch.nn.functional as F

from split_bounds import C_EPI, EPS

A_ACC = 56.0
H_MAX = 65504.0


def draw(rng, shape, zero_frac=0.1, lo=-10, hi=4):
    """float64 array of fp16-representable values: magnitudes 2^U[lo, hi] rounded to fp16 (never an fp16 subnormal: the
    smallest normal is 2^-14), random signs, a share of exact zeros"""
    v = np.exp2(rng.uniform(lo, hi, size=shape)) * rng.choice([-1.0, 1.0], size=shape)
    v = v.astype(np.float16).astype(np.float64)
    v[rng.random(size=shape) < zero_frac] = 0.0
    assert np.all((v == 0) | (np.abs(v) >= 2.0 ** -14))
    return v


def layer_ref(x, w, scale=None, shift=None, res=None, relu=False, stride=1, pad=0, dil=1, out_f32=False):
    """x (N,Cin,H,W), w (Cout,Cin,R,S), res (N,Cout,Ho,Wo): float64 arrays; scale / shift (Cout,) or None.
    -> (ref64, bound), both (N,Cout,Ho,Wo) float64"""
    xt, wt = torch.from_numpy(np.ascontiguousarray(x)).double(), torch.from_numpy(np.ascontiguousarray(w)).double()
    acc = F.conv2d(xt, wt, None, stride, pad, dil).numpy()
    aacc = F.conv2d(xt.abs(), wt.abs(), None, stride, pad, dil).numpy()
    C = w.shape[0]
    sc = np.ones(C) if scale is None else np.asarray(scale, np.float64)
    sh = np.zeros(C) if shift is None else np.asarray(shift, np.float64)
    sc, sh = sc.reshape(1, C, 1, 1), sh.reshape(1, C, 1, 1)
    r = np.zeros_like(acc) if res is None else np.asarray(res, np.float64)
    ref = acc * sc + sh + r
    if relu:
        ref = np.maximum(ref, 0.0)
    bound = A_ACC * EPS * aacc * np.abs(sc) + C_EPI * EPS * (np.abs(acc * sc) + np.abs(sh) + np.abs(r))
    if not out_f32:
        bound = bound + 2.0 ** -11 * np.abs(ref) + 2.0 ** -25
    return ref, bound


def excess(got, ref, bound):
    """max over elements of |got - ref| / bound (<= 1 passes)"""
    return float((np.abs(np.asarray(got, np.float64) - ref) / bound).max())


def _im2col(x, R, S, stride, pad, dil):
    cols = F.unfold(torch.from_numpy(np.ascontiguousarray(x)).double(), (R, S), dilation=dil, padding=pad, stride=stride)
    return cols.numpy()          # (N, Cin*R*S, L), k order (ci, r, s)


def emulate(x, w, scale=None, shift=None, res=None, relu=False, stride=1, pad=0, dil=1, out_f32=False, fault=None):
    """numpy emulation of the kernel's arithmetic: fp16 operands, exact products, fp32 accumulation in 16-wide chunks, fp32
    epilogue, one rounding.  fault: None | "round_before_res" | "scale_after_round" | "drop_tap" | "fp16_acc"."""
    N, Cin, H, W = x.shape
    Cout, _, R, S = w.shape
    cols = _im2col(x, R, S, stride, pad, dil)                   # (N, K, L)
    wm = w.reshape(Cout, -1).copy()                            # (Cout, K) in the same (ci, r, s) order
    K = wm.shape[1]
    if fault == "drop_tap":
        keep = np.ones((Cin, R, S))
        keep[:, R - 1, S - 1] = 0.0                            # the last tap is never multiplied
        wm = wm * keep.reshape(1, -1)
    acc_t = np.float16 if fault == "fp16_acc" else np.float32
    acc = np.zeros((N, Cout, cols.shape[2]), acc_t)
    for k0 in range(0, K, 16):
        part = np.einsum("ck,nkl->ncl", wm[:, k0:k0 + 16], cols[:, k0:k0 + 16])      # float64: exact for 16 fp16 products
        acc = (acc + part.astype(acc_t)).astype(acc_t)
    Ho = (H + 2 * pad - dil * (R - 1) - 1) // stride + 1
    acc = acc.reshape(N, Cout, Ho, -1).astype(np.float32)
    f32 = np.float32
    sc = None if scale is None else np.asarray(scale, f32).reshape(1, Cout, 1, 1)
    sh = None if shift is None else np.asarray(shift, f32).reshape(1, Cout, 1, 1)
    if fault == "scale_after_round":
        acc = acc.astype(np.float16).astype(f32)
    v = acc if sc is None else (acc * sc).astype(f32)
    if sh is not None:
        v = (v + sh).astype(f32)
    if fault == "round_before_res":
        v = v.astype(np.float16).astype(f32)
    if res is not None:
        v = (v + np.asarray(res, f32)).astype(f32)
    if relu:
        v = np.maximum(v, f32(0))
    if out_f32:
        return v.astype(np.float64)
    return np.clip(v, -H_MAX, H_MAX).astype(np.float16).astype(np.float64)
