"""-m gpu numerics tests of the conv / norm / pooling HIP kernels against plain
PyTorch fp32 (CPU) references of the same op, and of the whole ModelBuilder
forward/backward against goldens generated from the reference model."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conftest import golden
from model_utils import formula_state_dict, net_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda"
CL = torch.channels_last


def K():
    from u2pl_amd import nn as Kn
    return Kn


def _close(a, b, rtol=2e-4, atol=2e-5, what=""):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    err = (a - b).abs().max().item()
    ref = b.abs().max().item()
    assert err <= atol + rtol * ref, f"{what}: max err {err:.3e} vs ref max {ref:.3e}"


CONV_CASES = [
    # Cin, Cout, k, stride, dil, H, bias
    (64, 64, 3, 1, 1, 33, False),
    (64, 128, 3, 1, 1, 21, False),
    (128, 128, 3, 2, 1, 33, False),     # layer2 stride-2 3x3
    (256, 512, 1, 2, 1, 33, False),     # layer2 downsample
    (256, 256, 3, 1, 2, 25, False),     # layer3 dilation 2
    (512, 512, 3, 1, 16, 25, False),    # layer4 multi-grid (halo larger than the map)
    (2048, 256, 3, 1, 36, 13, False),   # ASPP d36
    (1024, 256, 1, 1, 1, 17, False),
    (512, 256, 3, 1, 1, 19, True),      # decoder tower with bias
    (256, 19, 1, 1, 1, 19, True),       # classifier (narrow N)
    (3, 64, 3, 2, 1, 33, False),        # stem (im2col path)
    (1280, 256, 3, 1, 1, 9, False),
]


@pytest.fixture(params=[0, 2, 4], ids=["direct", "wino2", "wino4"])
def conv_algo(request):
    """every conv test runs on the direct implicit-GEMM kernel and with the 3x3 stride-1 layers forced onto
    the Winograd F(2x2) / F(4x4) path (min_gain 0: also the dilations the production policy leaves direct)"""
    Kn = K()
    saved = dict(Kn.CONV_ALGO)
    Kn.CONV_ALGO.update(wino=request.param, min_gain=0.0)
    yield request.param
    Kn.CONV_ALGO.update(saved)


@pytest.mark.parametrize("Cin,Cout,k,stride,dil,H,bias", CONV_CASES)
def test_conv2d_fwd_bwd_vs_torch(Cin, Cout, k, stride, dil, H, bias, conv_algo):
    Kn = K()
    if conv_algo and not (k == 3 and stride == 1 and Cin % 32 == 0):
        pytest.skip("layer is not Winograd-eligible: covered by the direct run")
    g = torch.Generator().manual_seed(Cin * 7 + Cout + k + dil)
    N, W = 2, H + 2
    pad = dil * (k // 2)
    x = torch.randn(N, Cin, H, W, generator=g)
    ref = nn.Conv2d(Cin, Cout, k, stride=stride, padding=pad, dilation=dil, bias=bias)
    with torch.no_grad():
        ref.weight.copy_(torch.randn(ref.weight.shape, generator=g) / (Cin * k * k) ** 0.5)
        if bias:
            ref.bias.copy_(torch.randn(Cout, generator=g))
    xr = x.clone().requires_grad_(True)
    yr = ref(xr)
    gy = torch.randn(yr.shape, generator=g)
    yr.backward(gy)
    mine = Kn.Conv2d(Cin, Cout, k, stride=stride, padding=pad, dilation=dil, bias=bias).to(DEV)
    with torch.no_grad():
        mine.weight.copy_(ref.weight.detach().to(DEV))
        if bias:
            mine.bias.copy_(ref.bias.detach().to(DEV))
    xd = x.to(DEV).contiguous(memory_format=CL).requires_grad_(Cin != 3)
    yd = mine(xd)
    assert yd.shape == yr.shape
    _close(yd, yr, what="fwd")
    yd.backward(gy.to(DEV).contiguous(memory_format=CL))
    if Cin != 3:
        _close(xd.grad, xr.grad, what="dgrad")
    _close(mine.weight.grad, ref.weight.grad, rtol=3e-4, what="wgrad")
    if bias:
        _close(mine.bias.grad, ref.bias.grad, rtol=3e-4, what="bgrad")


def test_winograd_accuracy_and_fused_bn_statistics():
    """Winograd F(2x2)/F(4x4) against a float64 convolution: F(2x2) is as accurate as the direct fp32 kernel,
    F(4x4) within the documented 8x of it; the fused BatchNorm statistics equal the stand-alone pass."""
    Kn = K()
    g = torch.Generator().manual_seed(5)
    N, C, O, H, W, d = 2, 256, 256, 49, 45, 2
    x = torch.randn(N, C, H, W, generator=g)
    w = torch.randn(O, C, 3, 3, generator=g) / (9 * C) ** 0.5
    ref = F.conv2d(x.double(), w.double(), padding=d, dilation=d)
    errs = {}
    saved = dict(Kn.CONV_ALGO)
    try:
        for algo in (0, 2, 4):
            Kn.CONV_ALGO.update(wino=algo, min_gain=0.0)
            conv = Kn.Conv2d(C, O, 3, padding=d, dilation=d, bias=False).to(DEV)
            with torch.no_grad():
                conv.weight.copy_(w.to(DEV))
            bn = Kn.BatchNorm2d(O).to(DEV)
            bn.train()
            xd = x.to(DEV).contiguous(memory_format=CL)
            y = conv(xd)
            errs[algo] = (y.cpu().double() - ref).abs().max().item()
            # conv -> BN with the statistics produced by the conv's epilogue / output transform
            out_fused = Kn.conv_bn(conv, bn, xd, relu=False)
            bn2 = Kn.BatchNorm2d(O).to(DEV)
            bn2.train()
            out_plain = bn2(conv(xd))
            _close(out_fused, out_plain, rtol=2e-5, atol=2e-6, what=f"fused stats algo {algo}")
            _close(bn.running_var, bn2.running_var, rtol=1e-5, atol=1e-7, what="running_var")
    finally:
        Kn.CONV_ALGO.update(saved)
    print("max abs error vs float64:", errs)
    assert errs[2] <= 2.0 * errs[0] + 1e-7
    assert errs[4] <= 40.0 * errs[0] + 1e-7 and errs[4] < 1e-4


@pytest.mark.parametrize("C,O,k,d,H,W", [(256, 256, 3, 2, 41, 37), (1024, 256, 1, 1, 49, 45), (256, 1024, 1, 1, 33, 33),
                                         (64, 64, 3, 1, 65, 61), (2048, 256, 3, 12, 25, 25)])
def test_split_fp32_products_are_as_accurate_as_the_fp32_matrix_instruction(C, O, k, d, H, W):
    """The default arithmetic of the fp32 convolutions (csrc/conv.hip BF == 3 / k_conv_wgrad_bf16 SP == 3): every operand
    split EXACTLY into three bf16 pieces, the six piece products of weight >= 2^-16 accumulated in fp32 on the bf16
    matrix cores.  Against a float64 convolution its forward, data-gradient and weight-gradient errors must not exceed
    those of v_mfma_f32_32x32x2_f32 (u2pl_conv_set_split(0)) on the same kernels by more than 25 % (measured: equal or
    lower on every shape), on the all-direct kernel where nothing but the product arithmetic differs."""
    from u2pl_amd import _lib
    Kn = K()
    L = _lib.lib().cdll
    g = torch.Generator().manual_seed(C + O + k + d)
    N = 2
    x = torch.randn(N, C, H, W, generator=g)
    w = torch.randn(O, C, k, k, generator=g) / (k * k * C) ** 0.5
    gy = torch.randn(N, O, H, W, generator=g)
    xd, wd = x.double().requires_grad_(True), w.double().requires_grad_(True)
    yd = F.conv2d(xd, wd, padding=d * (k // 2), dilation=d)
    yd.backward(gy.double())
    ref = dict(y=yd.detach(), dx=xd.grad, dw=wd.grad)
    saved, old = dict(Kn.CONV_ALGO), L.u2pl_conv_get_split()
    errs = {}
    try:
        Kn.CONV_ALGO.update(wino=0)
        for mode in (0, 1):
            L.u2pl_conv_set_split(mode)
            conv = Kn.Conv2d(C, O, k, padding=d * (k // 2), dilation=d, bias=False).to(DEV)
            with torch.no_grad():
                conv.weight.copy_(w.to(DEV))
            xg = x.to(DEV).contiguous(memory_format=CL).requires_grad_(True)
            y = conv(xg)
            y.backward(gy.to(DEV).contiguous(memory_format=CL))
            got = dict(y=y.detach(), dx=xg.grad, dw=conv.weight.grad)
            errs[mode] = {n: ((got[n].cpu().double() - ref[n]).abs().max() / ref[n].abs().max()).item() for n in ref}
    finally:
        L.u2pl_conv_set_split(old)
        Kn.CONV_ALGO.update(saved)
    print("relative max error vs float64 (0: fp32 MFMA, 1: split):", errs)
    for n in ("y", "dx", "dw"):
        assert errs[1][n] <= 1.25 * errs[0][n] + 1e-8, (n, errs)
        assert errs[1][n] < 1e-5, (n, errs)


@pytest.mark.parametrize("arith", ["fp16x2", "bf16x3"])
@pytest.mark.parametrize("kind", ["relu_heavy_tail", "mixed_magnitudes", "cancellation"])
@pytest.mark.parametrize("C,O,k,d,H,W", [(256, 256, 1, 1, 33, 29), (128, 128, 3, 1, 25, 25), (1024, 256, 1, 1, 21, 21)])
def test_split_fp32_products_on_adversarial_operands(kind, C, O, k, d, H, W, arith):
    """The split arithmetic away from N(0,1) data, forward / data gradient / weight gradient against
    float64, measured like fp32 arithmetic should be -- against the CONDITION of the sums, sum |a||b| -- and compared with the
    fp32 matrix instruction on the same kernels:
      relu_heavy_tail   post-ReLU activations: 60 % exact zeros, the rest |N(0,1)|^3 (a few values carry the sums)
      mixed_magnitudes  input channels scaled 10^U(-6, 6), the weights of a channel by the inverse: every product is O(1)
                        but each operand spans 12 decades inside one reduction (pieces of very different exponents).  The
                        three-product fp16 form (arith fp16x2, the default since round 6) scales each TENSOR by one power of two:
                        it keeps fp32 accuracy for elements down to 2^-16 of the tensor's maximum and an absolute error of
                        2^-40 of the maximum below that, so its case spans 4 decades (10^U(-2, 2))
                        under the same bound, and the 12-decade case is held to the documented absolute bound instead
      cancellation      weights +w, -w on neighbouring input channels with nearly equal activations: the sums are ~1e-4 of
                        their terms (the Winograd-domain weight gradient's regime)
    Dropped piece products are <= 2^-23 |ab| each, so the error bound is a small multiple of eps32 * sum |a||b| -- the bound of
    an fp32 dot product."""
    from u2pl_amd import _lib
    Kn = K()
    L = _lib.lib().cdll
    g = torch.Generator().manual_seed(len(kind) * 1000 + C + O + k)
    N = 2
    x = torch.randn(N, C, H, W, generator=g)
    w = torch.randn(O, C, k, k, generator=g) / (k * k * C) ** 0.5
    gy = torch.randn(N, O, H, W, generator=g)
    if kind == "relu_heavy_tail":
        x = torch.relu(x - 0.25) ** 3
        gy = gy * (torch.rand(gy.shape, generator=g) < 0.3)
    elif kind == "mixed_magnitudes":
        dec = 12 if arith == "bf16x3" else 4
        sc = 10.0 ** (torch.rand(C, generator=g) * dec - dec / 2)
        x = x * sc.view(1, C, 1, 1)
        w = w / sc.view(1, C, 1, 1)
    else:
        base = torch.randn(N, C // 2, H, W, generator=g)
        x = torch.stack((base, base * (1 + 1e-4 * torch.randn(base.shape, generator=g))), 2).reshape(N, C, H, W)
        wh = torch.randn(O, C // 2, k, k, generator=g) / (k * k * C) ** 0.5
        w = torch.stack((wh, -wh), 2).reshape(O, C, k, k)
    pad = d * (k // 2)
    xd, wd = x.double().requires_grad_(True), w.double().requires_grad_(True)
    yd = F.conv2d(xd, wd, padding=pad, dilation=d)
    yd.backward(gy.double())
    ref = dict(y=yd.detach(), dx=xd.grad, dw=wd.grad)
    # condition of each sum: the same convolutions on absolute values
    xa, wa = x.double().abs().requires_grad_(True), w.double().abs().requires_grad_(True)
    ya = F.conv2d(xa, wa, padding=pad, dilation=d)
    ya.backward(gy.double().abs())
    cond = dict(y=ya.detach(), dx=xa.grad, dw=wa.grad)
    saved, old, saved_h = dict(Kn.CONV_ALGO), L.u2pl_conv_get_split(), dict(Kn.CONV_H)
    errs = {}
    try:
        Kn.CONV_ALGO.update(wino=0)
        Kn.CONV_H["on"] = arith == "fp16x2"
        for mode in (0, 1):
            L.u2pl_conv_set_split(mode)
            conv = Kn.Conv2d(C, O, k, padding=pad, dilation=d, bias=False).to(DEV)
            with torch.no_grad():
                conv.weight.copy_(w.to(DEV))
            xg = x.to(DEV).contiguous(memory_format=CL).requires_grad_(True)
            y = conv(xg)
            y.backward(gy.to(DEV).contiguous(memory_format=CL))
            got = dict(y=y.detach(), dx=xg.grad, dw=conv.weight.grad)
            assert all(torch.isfinite(v).all() for v in got.values())
            # error in units of eps32 * sum |a||b| (the size of ONE fp32 rounding of the largest partial sum)
            errs[mode] = {n: ((got[n].cpu().double() - ref[n]).abs() / (cond[n] * 2.0 ** -24 + 1e-300)).max().item() for n in ref}
    finally:
        L.u2pl_conv_set_split(old)
        Kn.CONV_ALGO.update(saved)
        Kn.CONV_H.update(saved_h)
    print(kind, arith, "max error in eps32 * sum|a||b| (0: fp32 MFMA, 1: split):", errs)
    for n in ("y", "dx", "dw"):
        # an fp32 dot product of length K is good to ~sqrt(K) .. K roundings; both arithmetics measured 1 .. 30 here
        assert errs[1][n] <= 1.5 * errs[0][n] + 4.0, (kind, n, errs)
        assert errs[1][n] < 64.0, (kind, n, errs)
    if arith == "fp16x2" and kind == "mixed_magnitudes":
        # the 12-decade case of the default arithmetic, held to the documented element-wise bound (tests/split_bounds.py)
        _fp16x2_twelve_decades_elementwise(C, O, k, d, H, W, pad, g)


def _fp16x2_twelve_decades_elementwise(C, O, k, d, H, W, pad, g):
    import split_bounds as SB
    Kn = K()
    x = torch.randn(2, C, H, W, generator=g)
    w = torch.randn(O, C, k, k, generator=g) / (k * k * C) ** 0.5
    gy = torch.randn(2, O, H, W, generator=g)
    sc = 10.0 ** (torch.rand(C, generator=g) * 12 - 6)
    x, w = x * sc.view(1, C, 1, 1), w / sc.view(1, C, 1, 1)
    saved, saved_h = dict(Kn.CONV_ALGO), dict(Kn.CONV_H)
    try:
        Kn.CONV_ALGO.update(wino=0)
        Kn.CONV_H["on"] = True
        conv = Kn.Conv2d(C, O, k, padding=pad, dilation=d, bias=False).to(DEV)
        with torch.no_grad():
            conv.weight.copy_(w.to(DEV))
        xg = x.to(DEV).contiguous(memory_format=CL).requires_grad_(True)
        with SB.recorded_calls(Kn) as seen:
            y = conv(xg)
            y.backward(gy.to(DEV).contiguous(memory_format=CL))
            torch.cuda.synchronize()
        got = dict(y=y.detach(), dx=xg.grad, dw=conv.weight.grad)
    finally:
        Kn.CONV_ALGO.update(saved)
        Kn.CONV_H.update(saved_h)
    # the split-fp16 entry points ran (not the six-product or fp32 kernels)
    assert seen.get("u2pl_conv2d_fwd_wsh_f32") and seen.get("u2pl_conv2d_dgrad_wsh_f32") and seen.get("u2pl_conv2d_wgrad_h_f32"), \
        sorted(seen)
    ref = SB.conv_refs(x, w, gy, 1, pad, d)
    for n in ("y", "dx", "dw"):
        e = SB.excess(got[n], *ref[n])
        assert e <= 1.0, ("twelve decades, fp16x2", n, e)


def test_split_fp16_twelve_decades_inside_one_tensor_meet_the_documented_absolute_bound():
    """the case the per-tensor scale cannot serve at fp32 accuracy (channels scaled 10^U(-6, 6), weights by the inverse): every term
    still carries at most 2^-40 max|x| |w| + 2^-40 max|w| |x| + 2^-23 |x w| of error -- the documented floor, checked term-wise
    against float64"""
    Kn = K()
    saved, saved_h = dict(Kn.CONV_ALGO), dict(Kn.CONV_H)
    g = torch.Generator().manual_seed(77)
    N, C, O, H, W = 2, 256, 256, 19, 17
    sc = 10.0 ** (torch.rand(C, generator=g) * 12 - 6)
    x = torch.randn(N, C, H, W, generator=g) * sc.view(1, C, 1, 1)
    w = torch.randn(O, C, 1, 1, generator=g) / C ** 0.5 / sc.view(1, C, 1, 1)
    try:
        Kn.CONV_ALGO.update(wino=0)
        Kn.CONV_H["on"] = True
        conv = Kn.Conv2d(C, O, 1, bias=False).to(DEV)
        with torch.no_grad():
            conv.weight.copy_(w.to(DEV))
            y = conv(x.to(DEV).contiguous(memory_format=CL))
        ref = F.conv2d(x.double(), w.double())
        xa, wa = x.double().abs(), w.double().abs()
        bound = (2.0 ** -40 * (float(xa.max()) * F.conv2d(torch.ones_like(xa), wa) + float(wa.max()) * F.conv2d(xa, torch.ones_like(wa)))
                 + 2.0 ** -22 * F.conv2d(xa, wa))
        assert bool(((y.cpu().double() - ref).abs() <= bound).all())
        # the data and weight gradients (u2pl_conv2d_dgrad_wsh_f32 / u2pl_conv2d_wgrad_h_f32) and a Winograd 3x3 layer
        # (u2pl_gemm_batched_wsh_f32 / u2pl_wgrad_batched_h_f32) under the element-wise bound of tests/split_bounds.py
        import split_bounds as SB
        gy = torch.randn(N, O, H, W, generator=g)
        xg = x.to(DEV).contiguous(memory_format=CL).requires_grad_(True)
        with SB.recorded_calls(Kn) as seen:
            conv(xg).backward(gy.to(DEV).contiguous(memory_format=CL))
            torch.cuda.synchronize()
        assert seen.get("u2pl_conv2d_dgrad_wsh_f32") and seen.get("u2pl_conv2d_wgrad_h_f32"), sorted(seen)
        bnd = SB.conv_refs(x, w, gy)
        assert SB.excess(xg.grad, *bnd["dx"]) <= 1.0
        assert SB.excess(conv.weight.grad, *bnd["dw"]) <= 1.0
        Kn.CONV_ALGO.update(wino=4, min_gain=0.0)
        w3 = torch.randn(O, C, 3, 3, generator=g) / (9 * C) ** 0.5 / sc.view(1, C, 1, 1)
        conv3 = Kn.Conv2d(C, O, 3, padding=1, bias=False).to(DEV)
        with torch.no_grad():
            conv3.weight.copy_(w3.to(DEV))
        xg = x.to(DEV).contiguous(memory_format=CL).requires_grad_(True)
        with SB.recorded_calls(Kn) as seen:
            y3 = conv3(xg)
            y3.backward(gy.to(DEV).contiguous(memory_format=CL))
            torch.cuda.synchronize()
        # the Winograd split-fp16 kernels ran: forward + transposed component products and the Winograd-domain weight gradient
        assert len(seen.get("u2pl_gemm_batched_wsh_f32", ())) == 2 and seen.get("u2pl_wgrad_batched_h_f32"), sorted(seen)
        from u2pl_amd._lib import query
        nsplit = query("u2pl_wgrad_batched_splits", query("u2pl_wino_tiles", N, H, W, 1, 4), C, O, 36)
        assert SB.excess(y3, *SB.wino_conv(x, w3, 1, 4)) <= 1.0
        assert SB.excess(xg.grad, *SB.wino_conv(gy, w3.flip(2, 3).transpose(0, 1), 1, 4)) <= 1.0
        assert SB.excess(conv3.weight.grad, *SB.wino_wgrad(x, gy, 1, 4, nsplit)) <= 1.0
    finally:
        Kn.CONV_ALGO.update(saved)
        Kn.CONV_H.update(saved_h)


@pytest.mark.parametrize("drop", [False, True])
@pytest.mark.parametrize("conv_h", [True, False])
def test_batchnorm_backward_relu_mask_recomputed_from_x_has_the_saved_masks_bits(drop, conv_h):
    """y = relu(BN(x)) [* dropout scale] without a residual: the backward recomputes [y > 0] from x with the forward's own
    expression instead of reading y (round 6) -- input gradient, dgamma, dbeta identical to the saved-y form, train and eval mode"""
    Kn = K()
    saved = (Kn.RELU_MASK_FROM_X, dict(Kn.CONV_H))
    torch.manual_seed(12)
    C, N, H, W = 96, 3, 21, 19
    x0 = (torch.randn(N, C, H, W, device=DEV) * 2).contiguous(memory_format=CL)
    gy = torch.randn(N, C, H, W, device=DEV).contiguous(memory_format=CL)
    dscale = ((torch.rand(N, C, device=DEV) > 0.2).float() / 0.8) if drop else None
    res = {}
    try:
        Kn.CONV_H["on"] = conv_h
        for mode in ("train", "eval"):
            for flag in (True, False):
                Kn.RELU_MASK_FROM_X = flag
                torch.manual_seed(13)               # (the same parameters in both runs)
                bn = Kn.BatchNorm2d(C).to(DEV)
                with torch.no_grad():
                    bn.weight.normal_(1.0, 0.3)
                    bn.bias.normal_(0.0, 0.5)
                    bn.running_mean.normal_(0, 0.3)
                    bn.running_var.uniform_(0.5, 2.0)
                bn.train(mode == "train")
                x = x0.clone().requires_grad_(True)
                y = bn(x, relu=True, drop=dscale)
                y.backward(gy)
                torch.cuda.synchronize()
                res[(mode, flag)] = (y.detach().clone(), x.grad.clone(), bn.weight.grad.clone(), bn.bias.grad.clone())
            for a, b in zip(res[(mode, True)], res[(mode, False)]):
                assert torch.equal(a, b), mode
    finally:
        Kn.RELU_MASK_FROM_X = saved[0]
        Kn.CONV_H.update(saved[1])


def test_conv_large_pixel_count_splitk():
    """many pixels (split-K wgrad with several slabs) and M not a multiple of the tile"""
    Kn = K()
    g = torch.Generator().manual_seed(1)
    x = torch.randn(3, 64, 97, 101, generator=g)
    ref = nn.Conv2d(64, 64, 3, padding=1, bias=False)
    xr = x.clone().requires_grad_(True)
    yr = ref(xr)
    gy = torch.randn(yr.shape, generator=g)
    yr.backward(gy)
    mine = Kn.Conv2d(64, 64, 3, padding=1, bias=False).to(DEV)
    with torch.no_grad():
        mine.weight.copy_(ref.weight.detach().to(DEV))
    xd = x.to(DEV).contiguous(memory_format=CL).requires_grad_(True)
    yd = mine(xd)
    yd.backward(gy.to(DEV).contiguous(memory_format=CL))
    _close(yd, yr, what="fwd")
    _close(xd.grad, xr.grad, what="dgrad")
    _close(mine.weight.grad, ref.weight.grad, rtol=5e-4, what="wgrad")


@pytest.mark.parametrize("C,H,relu,res,drop", [(64, 17, True, False, False), (256, 9, True, True, False),
                                               (1280, 5, False, False, False), (256, 11, True, False, True),
                                               (2048, 3, True, True, True)])
def test_batchnorm_train_fwd_bwd_vs_torch(C, H, relu, res, drop):
    Kn = K()
    g = torch.Generator().manual_seed(C + H)
    N = 3
    x = torch.randn(N, C, H, H, generator=g) * 2 + 0.7
    r = torch.randn(N, C, H, H, generator=g) if res else None
    dm = ((torch.rand(N, C, generator=g) > 0.3).float() / 0.7) if drop else None
    ref = nn.BatchNorm2d(C)
    with torch.no_grad():
        ref.weight.copy_(torch.rand(C, generator=g) + 0.5)
        ref.bias.copy_(torch.randn(C, generator=g) * 0.1)
        ref.running_mean.copy_(torch.randn(C, generator=g) * 0.1)
    mine = Kn.BatchNorm2d(C).to(DEV)
    mine.load_state_dict(ref.state_dict())
    pivot, rv0 = ref.running_mean.double().clone(), ref.running_var.double().clone()
    xr = x.clone().requires_grad_(True)
    rr = r.clone().requires_grad_(True) if res else None
    yr = ref(xr)
    if res:
        yr = yr + rr
    if relu:
        yr = F.relu(yr)
    if drop:
        yr = yr * dm[:, :, None, None]
    gy = torch.randn(yr.shape, generator=g)
    yr.backward(gy)
    xd = x.to(DEV).contiguous(memory_format=CL).requires_grad_(True)
    rd = r.to(DEV).contiguous(memory_format=CL).requires_grad_(True) if res else None
    yd = mine(xd, res=rd, relu=relu, drop=dm.to(DEV) if drop else None)
    yd.backward(gy.to(DEV).contiguous(memory_format=CL))
    _close(yd, yr, what="fwd")
    _close(xd.grad, xr.grad, rtol=5e-4, what="dx")
    if res:
        _close(rd.grad, rr.grad, what="dres")
    _close(mine.weight.grad, ref.weight.grad, rtol=5e-4, atol=1e-4, what="dgamma")
    _close(mine.bias.grad, ref.bias.grad, rtol=5e-4, atol=1e-4, what="dbeta")
    _close(mine.running_mean, ref.running_mean, what="running_mean")
    _close(mine.running_var, ref.running_var, what="running_var")
    # ... and element-wise against float64 (tests/bn_bounds.py): the stand-alone statistics (M <= 64: the float64 few-row kernel)
    import bn_bounds as BB
    M = N * H * H
    rows = lambda t: t.detach().double().cpu().permute(0, 2, 3, 1).reshape(M, C)     # noqa: E731
    X = rows(x)
    L = None if M <= BB.SMALL_M else BB.L_standalone(M, C)
    mu, var = BB.stats_ref(X)
    e_mu, e_var, e1 = BB.stats_bound(X, pivot, L)
    iota, e_iota, hi = BB.invstd_interval(var, e_var, float(np.float32(mine.eps)))
    G, B = ref.weight.detach().double(), ref.bias.detach().double()
    DR = dm.double().repeat_interleave(H * H, 0) if drop else None
    pre, b = BB.apply_ref_bound(X, mu, iota, e_mu, e_iota, hi, G, B, rows(r) if res else None)
    y64, by = BB.finish_y(pre, b, relu, DR)
    Y = rows(yd)
    assert BB.excess(Y, y64, by) <= 1.0
    assert not relu or BB.mask_mismatch(pre, b, Y, DR) == 0
    rm64, brm, rv64, brv = BB.running_ref_bound(pivot, rv0, mu, var, M, mine.momentum, e1, e_var)
    assert BB.excess(mine.running_mean, rm64, brm) <= 1.0 and BB.excess(mine.running_var, rv64, brv) <= 1.0
    bw = BB.bwd_ref_bound(X, rows(gy), (Y > 0).double() if relu else 1.0, DR, mu, iota, e_mu, e_iota, hi, G,
                          BB.L_colreduce_chain(M, C))
    assert BB.excess(rows(xd.grad), *bw["dx"]) <= 1.0
    if res:
        assert BB.excess(rows(rd.grad), *bw["dres"]) <= 1.0
    for got, (S, e) in ((mine.weight.grad, bw["S1"]), (mine.bias.grad, bw["S0"])):
        assert BB.excess(got, S, e * (1 + BB.EPS) + BB.EPS * S.abs()) <= 1.0
    # eval mode
    ref.eval(), mine.eval()
    _close(mine(xd.detach()), ref(x), what="eval fwd")


def test_batchnorm_on_channel_slice_and_single_pixel():
    Kn = K()
    g = torch.Generator().manual_seed(5)
    big = torch.randn(2, 512, 7, 7, generator=g).to(DEV).contiguous(memory_format=CL)
    sl = big[:, 128:384]
    ref = nn.BatchNorm2d(256)
    mine = Kn.BatchNorm2d(256).to(DEV)
    _close(mine(sl, relu=True), F.relu(ref(sl.cpu().contiguous())), what="slice")
    x1 = torch.randn(4, 256, 1, 1, generator=g)
    ref2, mine2 = nn.BatchNorm2d(256), Kn.BatchNorm2d(256).to(DEV)
    _close(mine2(x1.to(DEV), relu=True), F.relu(ref2(x1)), what="1x1")


def test_batchnorm_residual_gradient_without_input_gradient_is_an_error():
    """dres is written by the launch that writes dx: asking for the residual's gradient alone must raise, not hand autograd an
    unwritten buffer (the models never ask: a residual goes into a BatchNorm whose input is a convolution's output)"""
    Kn = K()
    from u2pl_amd._lib import HipError
    g = torch.Generator().manual_seed(6)
    x = torch.randn(2, 64, 9, 9, generator=g).to(DEV).contiguous(memory_format=CL)
    r = torch.randn(2, 64, 9, 9, generator=g).to(DEV).contiguous(memory_format=CL).requires_grad_(True)
    y = Kn.BatchNorm2d(64).to(DEV)(x, res=r, relu=True)
    with pytest.raises(HipError):
        y.sum().backward()


@pytest.mark.parametrize("H,W", [(33, 35), (65, 65), (385, 385)])
def test_maxpool_ceil_vs_torch(H, W):
    Kn = K()
    g = torch.Generator().manual_seed(H)
    x = torch.randn(2, 128, H, W, generator=g)
    x[0, :, 3, 3] = x[0, :, 3, 4]  # ties
    xr = x.clone().requires_grad_(True)
    yr = F.max_pool2d(xr, 3, 2, 1, ceil_mode=True)
    gy = torch.randn(yr.shape, generator=g)
    yr.backward(gy)
    xd = x.to(DEV).contiguous(memory_format=CL).requires_grad_(True)
    yd = Kn.MaxPool3x3s2Ceil()(xd)
    assert yd.shape == yr.shape
    yd.backward(gy.to(DEV).contiguous(memory_format=CL))
    assert torch.equal(yd.cpu(), yr.detach())
    _close(xd.grad, xr.grad, rtol=1e-6, atol=1e-6, what="maxpool bwd")


def test_gap_broadcast_upsample_cat():
    Kn = K()
    g = torch.Generator().manual_seed(9)
    x = torch.randn(2, 256, 17, 19, generator=g)
    xr = x.clone().requires_grad_(True)
    pr = F.adaptive_avg_pool2d(xr, 1)
    ur = F.interpolate(pr, (17, 19), mode="bilinear", align_corners=True)
    u2r = F.interpolate(xr, (65, 73), mode="bilinear", align_corners=True)  # >= 65 wide: torch's vectorised FMA path
    cr = torch.cat((ur, xr), 1)
    gc = torch.randn(cr.shape, generator=g)
    g2 = torch.randn(u2r.shape, generator=g)
    (cr * gc).sum().backward(retain_graph=True)
    (u2r * g2).sum().backward()
    xd = x.to(DEV).contiguous(memory_format=CL).requires_grad_(True)
    pd = Kn.global_avg_pool(xd)
    ud = Kn.upsample_bilinear(pd, (17, 19))
    u2d = Kn.upsample_bilinear(xd, (65, 73))
    cd = Kn.cat_channels((ud, xd))
    _close(pd, pr, what="gap")
    _close(cd, cr, what="cat")
    assert torch.equal(u2d.cpu(), u2r.detach()), "feature bilinear must be bit-exact (FMA form)"
    (cd * gc.to(DEV)).sum().backward(retain_graph=True)
    (u2d * g2.to(DEV)).sum().backward()
    _close(xd.grad, xr.grad, rtol=3e-4, what="combined backward")


def test_sgd_ema_arena_golden():
    from u2pl_amd.nn import ParamArena
    g = golden("sgd_ema")
    s = [nn.Parameter(torch.from_numpy(g["p0"]).to(DEV)), nn.Parameter(torch.from_numpy(g["p1"]).to(DEV))]
    t = [nn.Parameter(torch.from_numpy(g["t0"]).to(DEV)), nn.Parameter(torch.from_numpy(g["t1"]).to(DEV))]
    sa, ta = ParamArena([[s[0]], [s[1]]]), ParamArena([[t[0]], [t[1]]], with_grad=False)
    for it in range(6):
        sa.zero_grad()
        s[0].grad.copy_(torch.from_numpy(g[f"g0_{it}"]).to(DEV))
        s[1].grad.copy_(torch.from_numpy(g[f"g1_{it}"]).to(DEV))
        sa.sgd_step([float(x) for x in g[f"lr_{it}"]], 0.9, 0.0005)
        ta.ema_from(sa, float(g[f"ema_{it}"]))
        for j in range(2):
            assert np.abs(s[j].detach().cpu().numpy() - g[f"s{j}_{it}"]).max() < 1e-6
            assert np.abs(t[j].detach().cpu().numpy() - g[f"t{j}_{it}"]).max() < 1e-6


def _as_accurate(mine, ref32, ref64, what, slack=4.0, floor=1e-6, outlier_frac=0.0, scale_hint=0.0):
    """HIP result must be as close to the float64 ground truth as the reference's own
    fp32 path is (within `slack`x).  `outlier_frac` tolerates the few weight-gradient
    entries that change discretely when a near-zero pre-activation flips its ReLU
    (the reference's fp32 path shows the same sensitivity against its float64 twin).
    `scale_hint`: magnitude of the WHOLE tensor when `mine` is a sample of it -- the sample of a 3x3 weight gradient
    (every 1152nd entry = always tap (0, 0)) is structurally zero when that tap only ever sees padding (ASPP d=36 on a
    9x9 map); slack x 0 + floor x 0 would then demand bit-exact zeros, which a Winograd-domain gradient (a sum of
    component products that cancel) cannot promise in any arithmetic: the floor is relative to the tensor, not the sample."""
    mine, ref32, ref64 = (t.detach().cpu().double() for t in (mine, ref32, ref64))
    err = (mine - ref64).abs()
    e_ref = (ref32 - ref64).abs().max().item()
    scale = max(ref64.abs().max().item(), float(scale_hint))
    bad = (err > slack * e_ref + floor * scale).double().mean().item()
    e_mine = err.max().item()
    assert bad <= outlier_frac, f"{what}: |hip-f64|={e_mine:.3e} |ref32-f64|={e_ref:.3e} scale={scale:.3e} bad={bad:.4f}"
    return e_mine, e_ref


@pytest.mark.parametrize("tag,arch,S,C,aux", [("r50_65", "resnet50", 65, 19, True), ("r101_33", "resnet101", 33, 21, False)])
def test_model_builder_vs_reference_golden(tag, arch, S, C, aux, conv_algo):
    """Whole ModelBuilder (train-mode fwd, bwd, buffers, eval fwd) vs the reference model
    (formula weights, dropout ON with the keyed keep-masks the golden was written with).  Tolerance = the reference's own fp32
    error against its float64 twin, x4 -- for the direct kernel AND with every 3x3 layer forced onto Winograd
    F(2x2).  The F(4x4) run is a stress case: EVERY stride-1 3x3 layer (also the dilations the production
    policy keeps direct) on 9x9 / 5x5 maps of this deliberately ill-conditioned formula-weight network; its
    transforms cost ~7x the rounding error of a direct fp32 convolution per layer, so the bound there is x32
    (still three orders of magnitude below any indexing / transform mistake).  The production configuration
    (real initialisation, policy-selected layers) is held to the 1e-4 loss tolerance by test_gpu_train_step."""
    from u2pl_amd.models.model_helper import ModelBuilder
    slack, buf_rtol, extra_out = (32.0, 2e-3, 0.05) if conv_algo == 4 else (4.0, 1e-4, 0.0)
    g = golden("model_" + tag)
    model = ModelBuilder(net_cfg(arch, C, aux))
    model.load_state_dict(formula_state_dict(model))
    from oracle.parity_dropout import KeyedMasks, tag_model
    from u2pl_amd import nn as Kn
    tag_model(model, "student")
    assert all(m.p == 0.1 for m in model.modules() if isinstance(m, nn.Dropout2d))
    model = model.to(DEV)
    model.train()
    x = torch.from_numpy(g["x"]).to(DEV)
    Kn.DROPOUT_HOOK = KeyedMasks(int(g["dropout_seed"])).hook
    try:
        out = model(x)
    finally:
        Kn.DROPOUT_HOOK = None
    report = {}
    fails = []

    def chk(mine, k32, k64, what, outlier_frac=0.0, scale_hint=0.0):
        try:
            report[what] = _as_accurate(mine, torch.from_numpy(g[k32]), torch.from_numpy(g[k64]), what, slack=slack,
                                        outlier_frac=outlier_frac + extra_out, scale_hint=scale_hint)
        except AssertionError as e:
            fails.append(str(e))

    chk(out["pred"], "pred", "pred64", "pred")
    chk(out["rep"], "rep", "rep64", "rep")
    loss = (out["pred"] * torch.from_numpy(g["gp"]).to(DEV)).sum() + (out["rep"] * torch.from_numpy(g["gr"]).to(DEV)).sum()
    if aux:
        chk(out["aux"], "aux", "aux64", "aux")
        loss = loss + (out["aux"] * torch.from_numpy(g["ga"]).to(DEV)).sum()
    loss.backward()
    params = dict(model.named_parameters())
    for n in g["grad_names"]:
        n = str(n)
        gr = params[n].grad.detach().cpu().contiguous().flatten()
        sub = gr[:: max(1, gr.numel() // 4096)][:4096]
        chk(sub, "grad__" + n, "grad64__" + n, "grad " + n, outlier_frac=0.02, scale_hint=gr.abs().max().item())
    bufs = dict(model.named_buffers())
    for k in g.files:
        if k.startswith("buf__"):
            _close(bufs[k[5:]], torch.from_numpy(g[k]), rtol=buf_rtol, atol=1e-5, what=k)
    model.eval()
    with torch.no_grad():
        oe = model(x)
    chk(oe["pred"], "pred_eval", "pred_eval64", "pred_eval")
    chk(oe["rep"], "rep_eval", "rep_eval64", "rep_eval")
    # the no-grad eval forward above ran every conv -> BN (-> +identity -> ReLU) chain in the conv epilogue / Winograd
    # output transform (nn.conv_bn_eval); the two-kernel form (conv, then u2pl_bn_apply_f32) must give the same BITS
    assert Kn.FUSE_EVAL_BN
    Kn.FUSE_EVAL_BN = False
    try:
        with torch.no_grad():
            ou = model(x)
    finally:
        Kn.FUSE_EVAL_BN = True
    for k_ in ("pred", "rep") + (("aux",) if aux else ()):
        assert torch.equal(ou[k_], oe[k_]), f"fused eval-BN epilogue changed {k_}: max diff {(ou[k_] - oe[k_]).abs().max().item():.3e}"
    print("\n".join(f"{k}: hip {v[0]:.3e} ref32 {v[1]:.3e}" for k, v in report.items()))
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("N,Cin,Cout,H,d", [(4, 256, 256, 97, 2), (4, 512, 256, 193, 1), (2, 2048, 256, 97, 12)])
def test_full_size_winograd_agrees_with_direct_kernel(N, Cin, Cout, H, d):
    """BASELINE-size layers (layer3 3x3 d=2, decoder 512->256 @193^2, ASPP d=12): the Winograd F(4x4) path and the
    direct implicit-GEMM kernel agree on forward, data gradient and weight gradient, and the forward is linear
    (size-independent properties; a CPU reference at these sizes would take minutes)."""
    Kn = K()
    g = torch.Generator(device=DEV).manual_seed(11)
    x = torch.randn(N, Cin, H, H, device=DEV, generator=g).contiguous(memory_format=CL)
    x2 = torch.randn(N, Cin, H, H, device=DEV, generator=g).contiguous(memory_format=CL)
    gy = torch.randn(N, Cout, H, H, device=DEV, generator=g).contiguous(memory_format=CL)
    conv = Kn.Conv2d(Cin, Cout, 3, padding=d, dilation=d, bias=False).to(DEV)
    saved = dict(Kn.CONV_ALGO)
    res = {}
    try:
        for algo in (0, 4):
            Kn.CONV_ALGO.update(wino=algo, min_gain=0.0)
            xi = x.clone().requires_grad_(True)
            conv.weight.grad = None
            y = conv(xi)
            y.backward(gy)
            res[algo] = (y.detach(), xi.grad.detach(), conv.weight.grad.detach().clone())
        Kn.CONV_ALGO.update(wino=4, min_gain=0.0)
        with torch.no_grad():
            lin = conv(2.0 * x - 0.5 * x2) - (2.0 * conv(x) - 0.5 * conv(x2))
    finally:
        Kn.CONV_ALGO.update(saved)
    for name, a, b in zip(("fwd", "dgrad", "wgrad"), res[4], res[0]):
        scale = b.abs().max().item()
        err = (a - b).abs().max().item()
        print(name, "max |wino - direct|", err, "scale", scale)
        assert err <= 2e-4 * scale, (name, err, scale)
    assert lin.abs().max().item() <= 2e-4 * res[0][0].abs().max().item()


# ------------------------------------------------------------------ config 5: bf16-operand products
BF16_CASES = [
    # Cin, Cout, k, stride, dil, H, bias, N
    (256, 256, 3, 1, 2, 49, False, 2),
    (1024, 256, 1, 1, 1, 33, False, 3),
    (128, 128, 3, 2, 1, 33, False, 2),     # strided
    (512, 256, 3, 1, 1, 41, True, 2),
    (256, 19, 1, 1, 1, 29, True, 2),       # narrow head (padded gradient columns)
    (2048, 256, 3, 1, 12, 25, False, 2),   # ASPP
    (64, 64, 3, 1, 1, 37, False, 2),       # 64-wide tiles
]


@pytest.mark.parametrize("Cin,Cout,k,stride,dil,H,bias,N", BF16_CASES)
def test_bf16_operand_conv_matches_bf16_rounded_reference(Cin, Cout, k, stride, dil, H, bias, N):
    """U2PL_CONV_BF16 (BASELINE configs[4]): forward, data gradient and weight gradient with operands rounded to bf16
    (RNE) in LDS + fp32 accumulation == an fp32 convolution of the bf16-ROUNDED tensors (torch CPU), to fp32
    summation-order accuracy; the teacher-style call (no gradient recorded) stays on the fp32 kernel."""
    Kn = K()
    saved = dict(Kn.CONV_ALGO)
    Kn.CONV_ALGO.update(bf16=1)
    try:
        g = torch.Generator().manual_seed(Cin + Cout + k + H)
        W = H + 3
        pad = dil * (k // 2)
        rb = lambda t: t.bfloat16().float()
        x = torch.randn(N, Cin, H, W, generator=g)
        ref = nn.Conv2d(Cin, Cout, k, stride=stride, padding=pad, dilation=dil, bias=bias)
        with torch.no_grad():
            ref.weight.copy_(torch.randn(ref.weight.shape, generator=g) / (Cin * k * k) ** 0.5)
            if bias:
                ref.bias.copy_(torch.randn(Cout, generator=g))
        w = ref.weight.detach().clone()
        # forward reference: conv(bf16(x), bf16(w)) + bias in fp32
        yr = F.conv2d(rb(x), rb(w), ref.bias.detach() if bias else None, stride=stride, padding=pad, dilation=dil)
        gy = torch.randn(yr.shape, generator=g)
        # backward references: dgrad = conv_transpose(bf16(gy), bf16(w)); wgrad = corr(bf16(gy), bf16(x)); bias grad in fp32
        xr = rb(x).requires_grad_(True)
        wr = rb(w).requires_grad_(True)
        F.conv2d(xr, wr.detach(), None, stride=stride, padding=pad, dilation=dil).backward(rb(gy))
        F.conv2d(xr.detach(), wr, None, stride=stride, padding=pad, dilation=dil).backward(rb(gy))
        mine = Kn.Conv2d(Cin, Cout, k, stride=stride, padding=pad, dilation=dil, bias=bias).to(DEV)
        with torch.no_grad():
            mine.weight.copy_(w.to(DEV))
            if bias:
                mine.bias.copy_(ref.bias.detach().to(DEV))
        xd = x.to(DEV).contiguous(memory_format=CL).requires_grad_(True)
        yd = mine(xd)
        _close(yd, yr, rtol=2e-5, atol=2e-5, what="bf16 fwd")
        yd.backward(gy.to(DEV).contiguous(memory_format=CL))
        _close(xd.grad, xr.grad, rtol=2e-5, atol=2e-5, what="bf16 dgrad")
        _close(mine.weight.grad, wr.grad, rtol=5e-5, atol=5e-5, what="bf16 wgrad")
        if bias:
            _close(mine.bias.grad, gy.sum(dim=(0, 2, 3)), rtol=3e-4, what="bgrad")
        # rounding really happened (vs the un-rounded fp32 product) and the no-grad call is the fp32 kernel
        y32 = F.conv2d(x, w, ref.bias.detach() if bias else None, stride=stride, padding=pad, dilation=dil)
        assert (yd.detach().cpu() - y32).abs().max() > 1e-4
        with torch.no_grad():
            yt = mine(x.to(DEV).contiguous(memory_format=CL))
        _close(yt, y32, what="teacher-style call stays fp32")
    finally:
        Kn.CONV_ALGO.update(saved)


def test_bf16_student_training_step_tracks_the_fp32_step():
    """one semi-supervised step with the bf16 student: finite, the three losses within 2 % of the fp32 step's (same
    weights / inputs / draws), teacher path bit-identical (pseudo labels equal)"""
    import numpy as np
    from u2pl_amd import configs
    from u2pl_amd.models.model_helper import ModelBuilder
    from u2pl_amd.trainer import SemiTrainer
    from u2pl_amd.utils.loss_helper import get_criterion
    Kn = K()
    S, B = 97, 2
    cfg = configs.cityscapes_semi(arch="resnet50", crop=S, batch_size=B, sync_bn=False, epochs=20)
    cfg["criterion"]["kwargs"]["min_kept"] = 4000
    cfg["trainer"]["contrastive"]["current_class_threshold"] = 0.055
    torch.manual_seed(0)
    sd = {k: v.detach().clone() for k, v in ModelBuilder(cfg["net"]).state_dict().items()}
    g = torch.Generator().manual_seed(4)
    il, iu = torch.randn(B, 3, S, S, generator=g).to(DEV), torch.randn(B, 3, S, S, generator=g).to(DEV)
    ll = torch.randint(0, 19, (B, S, S), generator=g).to(DEV)
    out = {}
    saved = dict(Kn.CONV_ALGO)
    try:
        for mode in (0, 1):
            Kn.CONV_ALGO.update(bf16=mode)
            model, teacher = ModelBuilder(cfg["net"]), ModelBuilder(cfg["net"])
            model.load_state_dict(sd), teacher.load_state_dict(sd)
            for m in list(model.modules()) + list(teacher.modules()):
                if isinstance(m, nn.Dropout2d):
                    m.p = 0.0      # (device RNG draws differ between the two runs; the comparison is about the conv arithmetic)
            tr = SemiTrainer(cfg, model.to(DEV), teacher.to(DEV), get_criterion(cfg), steps_per_epoch=5)
            np.random.seed(1), torch.manual_seed(1)
            dbg = {}
            m = tr.train_step(il, ll, iu, epoch=0, debug=dbg)
            out[mode] = ([float(v) for v in m.cpu()], dbg["label_u"].cpu())
    finally:
        Kn.CONV_ALGO.update(saved)
    print("fp32", out[0][0], "bf16", out[1][0])
    assert all(np.isfinite(out[1][0]))
    assert torch.equal(out[0][1], out[1][1])                     # teacher (fp32) pseudo labels identical
    for a, b in zip(out[0][0], out[1][0]):
        assert abs(a - b) <= 0.02 * max(1.0, abs(a)), (out[0][0], out[1][0])


def test_adam_step_matches_torch_adam():
    """u2pl_adam_step_f32 on the flat arena (three lr segments, weight decay, DDP mean folded in as grad_scale) against
    torch.optim.Adam on CPU (lr_helper.py:20-21 `optim.Adam(parms, **kwargs)`) over five steps, at beta2 = 0.99 and at torch's
    default 0.999 (where a weight 1 - beta2 formed in fp32 would be 0.0009999871; tests/test_gpu_glue_bounds.py holds the
    moments element-wise to float64)"""
    from u2pl_amd.utils.lr_helper import get_optimizer
    for beta2 in (0.99, 0.999):
        g = torch.Generator().manual_seed(4)
        shapes = [(64, 32, 3, 3), (64,), (128, 64, 1, 1), (19, 128, 1, 1), (19,)]
        ref_p = [torch.nn.Parameter(torch.randn(s_, generator=g)) for s_ in shapes]
        our_p = [torch.nn.Parameter(p.detach().clone().to(DEV)) for p in ref_p]
        lrs = (1e-3, 1e-2, 5e-3)
        split = [ref_p[:2], ref_p[2:3], ref_p[3:]], [our_p[:2], our_p[2:3], our_p[3:]]
        kw = dict(lr=1e-3, betas=(0.9, beta2), eps=1e-8, weight_decay=1e-4)
        ref = torch.optim.Adam([dict(params=gr, lr=lr) for gr, lr in zip(split[0], lrs)], **kw)
        ours = get_optimizer([dict(params=gr, lr=lr) for gr, lr in zip(split[1], lrs)], dict(type="adam", kwargs=kw))
        for step in range(5):
            grads = [torch.randn(s_, generator=g) for s_ in shapes]
            ours.zero_grad()
            for p, q, gr in zip(ref_p, our_p, grads):
                p.grad = gr.clone()
                q._u2pl_grad.copy_(gr.to(DEV))
            ref.step()
            ours.step()
            for p, q in zip(ref_p, our_p):
                err = (q.detach().cpu() - p.detach()).abs().max().item()
                assert err <= 2e-6 * max(1.0, p.detach().abs().max().item()), (beta2, step, err)
        sd = ours.state_dict()
        assert float(sd["state"][0]["step"]) == 5.0
        rs = ref.state_dict()["state"]
        for i in range(len(shapes)):
            assert (sd["state"][i]["exp_avg"] - rs[i]["exp_avg"]).abs().max().item() <= 1e-6
            assert (sd["state"][i]["exp_avg_sq"] - rs[i]["exp_avg_sq"]).abs().max().item() <= 1e-6


def test_fused_batchnorm_launches_give_the_separate_launches_bits():
    """round 5: (1) ordered finish of the conv epilogue's partial statistics + finalisation in ONE launch, (2) the parameter
    gradients inside the backward-apply launch, (3) eval-mode 1 / sqrt(var + eps) of a whole model in one launch -- each
    against the separate launches it replaces (U2PL_NO_BN_FINISH_FUSION=1): outputs, input / parameter gradients and
    running statistics BIT-identical, train mode with residual + ReLU + dropout scale, and an eval-mode stack."""
    from u2pl_amd import nn as Kn
    saved = Kn.FUSE_BN_FINISH
    outs = []
    try:
        for fused in (True, False):
            Kn.FUSE_BN_FINISH = fused
            torch.manual_seed(3)
            conv = Kn.Conv2d(256, 384, 1, bias=False).to(DEV)
            bn = Kn.BatchNorm2d(384).to(DEV)
            conv2 = Kn.Conv2d(384, 128, 3, padding=1, bias=False).to(DEV)
            bn2 = Kn.BatchNorm2d(128).to(DEV)
            arena = Kn.ParamArena([list(conv.parameters()) + list(bn.parameters()) + list(conv2.parameters()) + list(bn2.parameters())])
            with torch.no_grad():
                bn.weight.normal_(1.0, 0.2), bn.bias.normal_(0, 0.2), bn.running_mean.normal_(0, 0.1)
            g = torch.Generator(device=DEV).manual_seed(9)
            x = torch.randn(2, 256, 23, 19, device=DEV, generator=g).contiguous(memory_format=CL).requires_grad_(True)
            r = torch.randn(2, 384, 23, 19, device=DEV, generator=g).contiguous(memory_format=CL).requires_grad_(True)
            drop = (torch.rand(2, 384, device=DEV, generator=g) > 0.1).float() / 0.9
            arena.zero_grad()
            y = Kn.conv_bn(conv, bn, x, res=r, relu=True, drop=drop)
            z = Kn.conv_bn(conv2, bn2, y, relu=True)
            gz = torch.randn(z.shape, device=DEV, generator=g).contiguous(memory_format=CL)
            z.backward(gz)
            Kn.wgrad_stream_sync()
            bn.eval(), bn2.eval()
            with torch.no_grad(), Kn.eval_invstd(torch.nn.ModuleList([bn, bn2])):
                e = Kn.conv_bn(conv2, bn2, Kn.conv_bn(conv, bn, x.detach(), res=r.detach(), relu=True), relu=True)
            torch.cuda.synchronize()
            outs.append([t.detach().clone() for t in (y, z, x.grad, r.grad, arena.grad, bn.running_mean, bn.running_var,
                                                      bn2.running_mean, bn2.running_var, e)])
    finally:
        Kn.FUSE_BN_FINISH = saved
    names = "y z dx dres arena_grad rm1 rv1 rm2 rv2 eval".split()
    for n, a, b in zip(names, outs[0], outs[1]):
        assert torch.equal(a, b), n
    assert float(outs[0][4].abs().sum()) > 0


def test_residual_gradient_folded_into_conv1_dgrad_equals_autograd_add():
    """round 5: the block input's two gradient contributions (conv1's data gradient + the residual branch out of bn3's
    backward) summed inside conv1's data-gradient launch (forward kernel's epilogue with identity BatchNorm parameters and the
    residual gradient as `res`) instead of by autograd's elementwise add: same values (fl(a + b) either way) for the input
    gradient and every parameter gradient of two stacked bottlenecks; the first one has a downsample branch (not linked)."""
    from u2pl_amd import nn as Kn
    from u2pl_amd.models.resnet import Bottleneck
    saved = Kn.FUSE_RES_GRAD
    outs = []
    try:
        for fused in (True, False):
            Kn.FUSE_RES_GRAD = fused
            torch.manual_seed(11)
            ds = torch.nn.Sequential(Kn.Conv2d(256, 512, 1, bias=False), Kn.BatchNorm2d(512))
            blocks = torch.nn.Sequential(Bottleneck(256, 128, downsample=ds), Bottleneck(512, 128), Bottleneck(512, 128, dilation=2)).to(DEV)
            for m in blocks.modules():
                if isinstance(m, Kn.BatchNorm2d):
                    torch.nn.init.normal_(m.weight, 1.0, 0.2)
            arena = Kn.ParamArena([list(blocks.parameters())])
            g = torch.Generator(device=DEV).manual_seed(2)
            x = torch.randn(2, 256, 33, 29, device=DEV, generator=g).contiguous(memory_format=CL).requires_grad_(True)
            arena.zero_grad()
            y = blocks(x)
            gy = torch.randn(y.shape, device=DEV, generator=g).contiguous(memory_format=CL)
            y.backward(gy)
            Kn.wgrad_stream_sync()
            torch.cuda.synchronize()
            outs.append((y.detach().clone(), x.grad.clone(), arena.grad.clone()))
    finally:
        Kn.FUSE_RES_GRAD = saved
    for n, a, b in zip(("y", "dx", "param grads"), outs[0], outs[1]):
        assert torch.equal(a, b), (n, float((a - b).abs().max()))
    assert float(outs[0][1].abs().sum()) > 0


def test_gradient_joins_of_downsample_blocks_and_aspp_equal_autograd_sums():
    """nn.GradJoin beyond the plain residual: (1) a bottleneck WITH a (stride-1) downsample branch -- conv1 and the downsample conv
    both consume the block input: fl(a + b) either way, bit-equal; (2) the ASPP -- four convolutions consume the 2048-channel
    encoder output (pointwise, two Winograd, one direct 3x3): the chain adds the four contributions in another ORDER than
    autograd did, so equality holds to fp32 rounding of a four-term sum; the fifth consumer (global average pool) stays with
    autograd.  Input and parameter gradients against the un-joined path."""
    from u2pl_amd import nn as Kn
    from u2pl_amd.models.base import ASPP
    from u2pl_amd.models.resnet import Bottleneck
    saved = Kn.FUSE_RES_GRAD
    outs = []
    try:
        for fused in (True, False):
            Kn.FUSE_RES_GRAD = fused
            torch.manual_seed(13)
            ds = torch.nn.Sequential(Kn.Conv2d(256, 512, 1, bias=False), Kn.BatchNorm2d(512))
            block = Bottleneck(256, 128, downsample=ds, dilation=2).to(DEV)
            aspp = ASPP(512, inner_planes=256, dilations=(2, 12, 3)).to(DEV)       # at 25 x 25: d = 12 stays direct, d = 2 / 3 Winograd
            arena = Kn.ParamArena([list(block.parameters()) + list(aspp.parameters())])
            g = torch.Generator(device=DEV).manual_seed(4)
            x = torch.randn(2, 256, 25, 25, device=DEV, generator=g).contiguous(memory_format=CL).requires_grad_(True)
            arena.zero_grad()
            mid = block(x)
            y = aspp(mid)
            kinds = [bool(Kn.dgrad_fusable(b[0], mid)) for b in (aspp.conv2, aspp.conv3, aspp.conv4, aspp.conv5)]
            gy = torch.randn(y.shape, device=DEV, generator=g).contiguous(memory_format=CL)
            y.backward(gy)
            Kn.wgrad_stream_sync()
            torch.cuda.synchronize()
            outs.append((y.detach().clone(), x.grad.clone(), arena.grad.clone()))
    finally:
        Kn.FUSE_RES_GRAD = saved
    assert kinds == [True, True, False, True], kinds          # the case exercises both the fused forms and the in-place fallback
    assert torch.equal(outs[0][0], outs[1][0])
    for n, a, b in zip(("dx", "param grads"), outs[0][1:], outs[1][1:]):
        scale = float(b.abs().max())
        assert float((a - b).abs().max()) <= 2e-6 * scale, (n, float((a - b).abs().max()), scale)
