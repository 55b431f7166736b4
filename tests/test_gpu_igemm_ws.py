"""-m gpu: the pre-split-weight GEMM (csrc/igemm_ws.hip) against conv.hip's in-loop split kernels.

Both compute the split-fp32 product with the same six piece products in the same order, so every output -- forward,
fused BatchNorm statistics, fused eval-mode BatchNorm, data gradient, Winograd component batches -- must be the SAME
BITS (the conv.hip kernels themselves are checked against torch fp32 / float64 in test_gpu_conv_stack.py).  Plus the
once-per-step operand cache: a cached split must be rebuilt when the arena optimizer or a torch in-place op changes the
weight, and only then."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import split_bounds as SB  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
CL = torch.channels_last


def K():
    from u2pl_amd import nn as Kn
    return Kn


@pytest.fixture
def ws_switch():
    """the six-product bf16 form (U2PL_CONV_H=0): the arithmetic the pre-split kernels share bit for bit with conv.hip's in-loop
    split.  The three-product fp16 form (the default since round 6) has its own tests at the end of this file (wsh_switch)."""
    Kn = K()
    saved = (dict(Kn.CONV_ALGO), dict(Kn.CONV_WS), dict(Kn.CONV_H))
    Kn.CONV_H["on"] = False
    yield Kn
    Kn.CONV_ALGO.update(saved[0])
    Kn.CONV_WS.update(saved[1])
    Kn.CONV_H.update(saved[2])


@pytest.fixture
def wsh_switch():
    Kn = K()
    saved = (dict(Kn.CONV_ALGO), dict(Kn.CONV_WS), dict(Kn.CONV_H))
    Kn.CONV_H["on"] = True
    Kn.CONV_WS["on"] = True
    yield Kn
    Kn.CONV_ALGO.update(saved[0])
    Kn.CONV_WS.update(saved[1])
    Kn.CONV_H.update(saved[2])


# Cin, Cout, k, stride, dil, H, W, N, bias        (Cout > 64: the layers the ws kernel serves)
CASES = [
    (1024, 256, 1, 1, 1, 33, 29, 2, False),     # layer3 conv1: pointwise, one 256-wide column tile
    (256, 1024, 1, 1, 1, 33, 29, 2, False),     # layer3 conv3: four column tiles
    (512, 128, 1, 1, 1, 25, 25, 2, False),      # layer2 conv1: the 128-wide tile
    (256, 512, 1, 2, 1, 33, 33, 2, False),      # layer2 downsample: strided gather (not pointwise)
    (128, 128, 3, 2, 1, 33, 33, 1, False),      # stride-2 3x3
    (512, 256, 3, 1, 12, 25, 21, 1, True),      # ASPP-like dilated 3x3 with bias, halo > map on one side
    (2048, 256, 3, 1, 36, 13, 13, 1, False),    # ASPP d36
    (320, 320, 1, 1, 1, 19, 17, 1, True),       # Cout not a multiple of the tile, rows padded in the split planes
    (64, 256, 1, 1, 1, 40, 40, 1, False),       # K = 64: two chunks (prologue / clamped prefetch only)
    (32, 96, 1, 1, 1, 21, 21, 1, False),        # K = 32: a single chunk
    (128, 130, 1, 1, 1, 23, 19, 1, True),       # Cout not a multiple of 4
    (128, 256, 3, 1, 5, 40, 23, 3, False),      # filter-row skipping: tiles that straddle image boundaries, 5 of 40 rows per side
    (256, 192, 3, 1, 24, 33, 29, 2, True),      # filter-row skipping: r = 0 / r = 2 outside for most tiles, both for none
    (512, 256, 1, 1, 1, 140, 140, 2, True),     # 307 wide tiles: the MIXED plan (256 wide + 102 narrow tiles in one launch), pointwise
    (64, 512, 3, 1, 2, 128, 80, 2, False),      # 320 wide tiles: the mixed plan on the gather kernel (dgrad: 512 -> 64 stays on conv.hip)
]


# the two cases of the table that are there for the mixed plan -> (kind, wide tiles, narrow tiles) of u2pl_igemm_ws_plan, forward
MIXED_CASES = {(512, 256, 1): (2, 256, 102), (64, 512, 3): (2, 256, 128)}
WS_PLAN_SWITCHES = ("U2PL_WS_NARROW", "U2PL_WS_MIX2", "U2PL_WS_FIX2", "U2PL_WS_PERSIST")


def _ws_plan(M, Kred, Cout, batch, np_):
    import ctypes
    from u2pl_amd._lib import lib
    out = (ctypes.c_int * 3)()
    assert lib().u2pl_igemm_ws_plan(M, Kred, Cout, batch, np_, out) == 0
    return tuple(out)


def _run(Kn, ws_on, conv, x, gy, pivot=None):
    Kn.CONV_WS["on"] = ws_on
    x = x.detach().clone().requires_grad_(True)
    conv.weight.grad = None
    if pivot is None:
        y = conv(x)
        sums = None
    else:
        y, sums = conv(x, stat_pivot=pivot)
        sums = Kn.finished_sums(sums, conv.out_channels)        # (the conv hands out its epilogue's raw partials since round 5)
    y.backward(gy)
    torch.cuda.synchronize()
    return y.detach(), x.grad.detach(), sums


@pytest.mark.parametrize("Cin,Cout,k,stride,dil,H,W,N,bias", CASES)
def test_ws_forward_dgrad_stats_bit_identical(Cin, Cout, k, stride, dil, H, W, N, bias, ws_switch):
    Kn = ws_switch
    Kn.CONV_ALGO.update(wino=0)
    torch.manual_seed(Cin * 7 + Cout + k + dil)
    conv = Kn.Conv2d(Cin, Cout, k, stride=stride, padding=dil * (k // 2), dilation=dil, bias=bias).to(DEV)
    x = torch.randn(N, Cin, H, W, device=DEV).contiguous(memory_format=CL)
    Ho = (H + 2 * dil * (k // 2) - dil * (k - 1) - 1) // stride + 1
    Wo = (W + 2 * dil * (k // 2) - dil * (k - 1) - 1) // stride + 1
    gy = torch.randn(N, Cout, Ho, Wo, device=DEV).contiguous(memory_format=CL)
    pivot = torch.randn(Cout, device=DEV) * 0.1
    if (Cin, Cout, k) in MIXED_CASES and not any(os.environ.get(v) for v in WS_PLAN_SWITCHES):
        assert _ws_plan(N * Ho * Wo, k * k * Cin, Cout, 1, 3) == MIXED_CASES[(Cin, Cout, k)]       # (what the table calls the mixed plan is)
    _check_case(Kn, conv, x, gy, pivot, Cout)


def _check_case(Kn, conv, x, gy, pivot, Cout):
    y0, dx0, _ = _run(Kn, False, conv, x, gy)
    y1, dx1, _ = _run(Kn, True, conv, x, gy)
    assert torch.equal(y0, y1), f"forward differs: {(y0 - y1).abs().max().item():.3e}"
    assert torch.equal(dx0, dx1), f"data gradient differs: {(dx0 - dx1).abs().max().item():.3e}"
    ys0, _, s0 = _run(Kn, False, conv, x, gy, pivot)
    ys1, _, s1 = _run(Kn, True, conv, x, gy, pivot)
    assert torch.equal(ys0, ys1) and torch.equal(ys0, y0)
    assert torch.equal(s0[: 2 * Cout], s1[: 2 * Cout]), "fused BatchNorm statistics differ"


@pytest.mark.parametrize("Cin,Cout,dil,H,W,N", [(256, 256, 2, 33, 29, 2), (512, 512, 4, 21, 21, 1), (128, 128, 1, 37, 37, 1)])
@pytest.mark.parametrize("mt", [4, 2])
def test_ws_winograd_component_batches_bit_identical(Cin, Cout, dil, H, W, N, mt, ws_switch):
    Kn = ws_switch
    Kn.CONV_ALGO.update(wino=mt, min_gain=0.0)
    torch.manual_seed(Cin + Cout + dil + mt)
    conv = Kn.Conv2d(Cin, Cout, 3, padding=dil, dilation=dil, bias=False).to(DEV)
    x = torch.randn(N, Cin, H, W, device=DEV).contiguous(memory_format=CL)
    gy = torch.randn(N, Cout, H, W, device=DEV).contiguous(memory_format=CL)
    y0, dx0, _ = _run(Kn, False, conv, x, gy)
    y1, dx1, _ = _run(Kn, True, conv, x, gy)
    assert torch.equal(y0, y1), f"Winograd forward differs: {(y0 - y1).abs().max().item():.3e}"
    assert torch.equal(dx0, dx1), f"Winograd data gradient differs: {(dx0 - dx1).abs().max().item():.3e}"


@pytest.mark.parametrize("res,relu", [(False, True), (True, True), (False, False)])
def test_ws_eval_batchnorm_epilogue_bit_identical(res, relu, ws_switch):
    Kn = ws_switch
    Kn.CONV_ALGO.update(wino=0)
    torch.manual_seed(5)
    conv = Kn.Conv2d(256, 384, 1, bias=False).to(DEV)
    bn = Kn.BatchNorm2d(384).to(DEV).eval()
    with torch.no_grad():
        bn.running_mean.normal_(0, 0.2)
        bn.running_var.uniform_(0.5, 2.0)
        bn.weight.normal_(1.0, 0.2)
        bn.bias.normal_(0, 0.2)
    x = torch.randn(2, 256, 27, 23, device=DEV).contiguous(memory_format=CL)
    r = torch.randn(2, 384, 27, 23, device=DEV).contiguous(memory_format=CL) if res else None
    outs = []
    with torch.no_grad():
        for on in (False, True):
            Kn.CONV_WS["on"] = on
            outs.append(Kn.conv_bn_eval(conv, bn, x, res=r, relu=relu))
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])


def test_ws_operand_cache_follows_the_weights(ws_switch):
    """the split planes are rebuilt when the weights change through the arena kernels (epoch) or through torch in-place
    ops (version) -- and reused otherwise"""
    Kn = ws_switch
    Kn.CONV_ALGO.update(wino=0)
    Kn.CONV_WS["on"] = True
    torch.manual_seed(11)
    conv = Kn.Conv2d(128, 256, 1, bias=False).to(DEV)
    arena = Kn.ParamArena([[conv.weight]])
    x = torch.randn(1, 128, 19, 19, device=DEV).contiguous(memory_format=CL)

    def fwd(on):
        Kn.CONV_WS["on"] = on
        with torch.no_grad():
            y = conv(x)
        torch.cuda.synchronize()
        return y

    y_a = fwd(True)
    ent = conv.weight._u2pl_derived["f"]
    stamp = ent["stamp"]
    assert torch.equal(fwd(True), y_a) and ent["stamp"] == stamp      # reused
    # arena SGD step (raw-pointer write: the epoch marks it)
    arena.grad.normal_(0, 1.0)
    arena.sgd_step([0.1], 0.9, 1e-4)
    y_b = fwd(True)
    assert ent["stamp"] != stamp
    assert not torch.equal(y_a, y_b)
    assert torch.equal(y_b, fwd(False)), "stale split planes after an arena optimizer step"
    # torch in-place write (load_state_dict / init paths: the version marks it)
    with torch.no_grad():
        conv.weight.mul_(0.5)
    y_c = fwd(True)
    assert torch.equal(y_c, fwd(False)), "stale split planes after a torch in-place update"
    assert not torch.equal(y_c, y_b)
    # a NEW weight that lands on a freed weight's address (same shape, same version) must not see the old planes
    conv2 = Kn.Conv2d(128, 256, 1, bias=False).to(DEV)
    w_old = conv2.weight.detach().clone()
    fwd2 = lambda on: (Kn.CONV_WS.update(on=on), conv2(x))[1]       # noqa: E731
    with torch.no_grad():
        y2 = fwd2(True)
        del conv2
        conv3 = Kn.Conv2d(128, 256, 1, bias=False).to(DEV)
        Kn.CONV_WS["on"] = True
        y3 = conv3(x)
        Kn.CONV_WS["on"] = False
        y3_ref = conv3(x)
    torch.cuda.synchronize()
    assert torch.equal(y3, y3_ref) and not torch.equal(y3, y2)


def test_presplit_rebuilds_every_operand_in_batched_launches_with_the_lazy_paths_bits(ws_switch):
    """ParamArena.sgd_step -> presplit: forward planes, transposed (data-gradient) planes and both Winograd filter forms of
    every weight the model used are rebuilt by ONE transform + ONE split launch and stamped current -- the next step's layer
    calls launch nothing -- and hold exactly the bytes the per-weight lazy path builds"""
    from u2pl_amd._lib import query
    Kn = ws_switch
    Kn.CONV_ALGO.update(wino=4, min_gain=0.0)
    Kn.CONV_WS["on"] = True
    saved = Kn.PRESPLIT["on"]
    torch.manual_seed(21)
    convs = [Kn.Conv2d(128, 256, 1, bias=False).to(DEV), Kn.Conv2d(256, 128, 3, padding=2, dilation=2, bias=False).to(DEV),
             Kn.Conv2d(128, 160, 3, stride=2, padding=1, bias=False).to(DEV), Kn.Conv2d(160, 96, 1, bias=True).to(DEV)]
    arena = Kn.ParamArena([[p for c in convs for p in c.parameters()]])
    x = torch.randn(2, 128, 21, 19, device=DEV).contiguous(memory_format=CL)

    def step():
        h = x.clone().requires_grad_(True)
        y = h
        for c in convs:
            y = c(y)
        y.square().mean().backward()
        torch.cuda.synchronize()
        return y.detach().clone(), h.grad.clone()

    try:
        Kn.PRESPLIT["on"] = False
        step()                                             # builds and registers every operand (lazy path)
        kinds = sorted(k for c in convs for k in c.weight._u2pl_derived)
        assert kinds == sorted(["f", "d", "wf4", "wd4", "f", "d", "f", "d"]), kinds
        arena.grad.normal_(0, 1.0)
        arena.sgd_step([0.05], 0.9, 1e-4)
        y_lazy, dx_lazy = step()                           # lazy rebuild after the update
        lazy = {(i, k): e["buf"].clone() for i, c in enumerate(convs) for k, e in c.weight._u2pl_derived.items()}
        # same update again from the same state, this time through presplit
        Kn.PRESPLIT["on"] = True
        for c in convs:
            for e in c.weight._u2pl_derived.values():
                e["buf"].zero_()
        Kn.bump_weight_epoch()
        k0 = query("u2pl_kernel_launches")
        n = Kn.presplit(arena.params, arena)
        assert n == 8 and query("u2pl_kernel_launches") - k0 == 2
        torch.cuda.synchronize()
        for (i, k), b in lazy.items():
            e = convs[i].weight._u2pl_derived[k]
            assert torch.equal(e["buf"], b), (i, k)
            assert e["stamp"] == Kn._weight_stamp(convs[i].weight)
        k1 = query("u2pl_kernel_launches")
        y_pre, dx_pre = step()
        assert torch.equal(y_pre, y_lazy) and torch.equal(dx_pre, dx_lazy)
        launches_pre = query("u2pl_kernel_launches") - k1
        Kn.PRESPLIT["on"] = False
        Kn.bump_weight_epoch()
        k2 = query("u2pl_kernel_launches")
        step()
        assert query("u2pl_kernel_launches") - k2 > launches_pre, "the lazy path should have launched the per-weight builds"
        # and through the arena hook
        Kn.PRESPLIT["on"] = True
        arena.grad.normal_(0, 1.0)
        arena.sgd_step([0.05], 0.9, 1e-4)
        for c in convs:
            for e in c.weight._u2pl_derived.values():
                assert e["stamp"] == Kn._weight_stamp(c.weight)
        y_a, dx_a = step()
        Kn.CONV_WS["on"] = False
        y_b, dx_b = step()
        assert torch.equal(y_a, y_b) and torch.equal(dx_a, dx_b)
        # another arena's update (the teacher's EMA beside the student's optimizer step) leaves these operands valid
        Kn.CONV_WS["on"] = True
        other = Kn.Conv2d(128, 256, 1, bias=False).to(DEV)
        arena2 = Kn.ParamArena([[other.weight]])
        with torch.no_grad():
            other(x)
        before = {(i, k): e["stamp"] for i, c in enumerate(convs) for k, e in c.weight._u2pl_derived.items()}
        arena2.grad.normal_(0, 1.0)
        arena2.sgd_step([0.05], 0.9, 1e-4)
        assert other.weight._u2pl_derived["f"]["stamp"] == Kn._weight_stamp(other.weight)
        for (i, k), st in before.items():
            assert st == Kn._weight_stamp(convs[i].weight) == convs[i].weight._u2pl_derived[k]["stamp"]
        k3 = query("u2pl_kernel_launches")
        step()
        assert query("u2pl_kernel_launches") - k3 == launches_pre
    finally:
        Kn.PRESPLIT["on"] = saved


def test_ws_nonfinite_operands_give_nonfinite_outputs(ws_switch):
    """documented semantics of the split arithmetic: an Inf or NaN operand makes every output
    it contributes to NaN (the fp32 matrix instruction would keep +-Inf for Inf * finite) -- never a finite value"""
    Kn = ws_switch
    Kn.CONV_ALGO.update(wino=0)
    torch.manual_seed(3)
    conv = Kn.Conv2d(64, 128, 1, bias=False).to(DEV)
    x = torch.randn(1, 64, 9, 9, device=DEV).contiguous(memory_format=CL)
    for on in (True, False):
        Kn.CONV_WS["on"] = on
        for bad in (float("inf"), float("-inf"), float("nan")):
            xx = x.clone()
            xx[0, 5, 3, 4] = bad
            with torch.no_grad():
                y = conv(xx)
            torch.cuda.synchronize()
            assert not torch.isfinite(y[0, :, 3, 4]).any(), "a non-finite input produced finite outputs"
            mask = torch.ones(9, 9, dtype=torch.bool, device=DEV)
            mask[3, 4] = False
            assert torch.isfinite(y[0][:, mask]).all(), "a non-finite input leaked into other pixels"
        with torch.no_grad():
            w0 = conv.weight[7, 9, 0, 0].item()
            conv.weight[7, 9, 0, 0] = float("inf")
            y = conv(x)
            conv.weight[7, 9, 0, 0] = w0
        torch.cuda.synchronize()
        assert not torch.isfinite(y[0, 7]).any() and torch.isfinite(y[0, :7]).all() and torch.isfinite(y[0, 8:]).all()


def test_ws_component_batch_larger_than_2gib_matches_the_in_loop_split_kernel():
    """only the per-MATRIX extents are limited to 2 GiB (32-bit offsets inside one matrix); a batch of 36
    Winograd components whose V buffer exceeds 2 GiB as a whole must run (the kernel rebuilds its descriptors per matrix from
    a 64-bit base) and give u2pl_gemm_batched_f32's bits in every component, including the ones past the 2 GiB mark."""
    from u2pl_amd._lib import call, query
    Kn = K()
    if query("u2pl_conv_get_split") != 1:
        pytest.skip("split-fp32 arithmetic is off")
    a2, tiles, Ci, Co = 36, 7424, 2048, 128           # V: 36 x 7424 x 2048 x 4 B = 2.19 GB; one matrix 60.8 MB
    assert a2 * tiles * Ci * 4 > (1 << 31)
    g = torch.Generator(device=DEV).manual_seed(5)
    V = torch.randn(a2 * tiles * Ci, device=DEV, generator=g)
    U = torch.randn(a2 * Co * Ci, device=DEV, generator=g) * 0.05
    M0 = torch.empty(a2 * tiles * Co, device=DEV)
    M1 = torch.full((a2 * tiles * Co,), float("nan"), device=DEV)
    call("u2pl_gemm_batched_f32", V, Ci, tiles * Ci, U, Co * Ci, M0, Co, tiles * Co, tiles, Ci, Co, a2)
    buf = torch.empty(query("u2pl_weight_split3_bytes", Co, Ci, a2), dtype=torch.uint8, device=DEV)
    call("u2pl_weight_split3_f32", U, Co * Ci, Co, Ci, a2, buf)
    call("u2pl_gemm_batched_ws_f32", V, Ci, tiles * Ci, buf, M1, Co, tiles * Co, tiles, Ci, Co, a2)
    torch.cuda.synchronize()
    assert torch.equal(M0, M1)
    assert float(M1.view(a2, -1)[-1].abs().max()) > 0


def test_split_guard_finite_operands_above_bf16_max_stay_finite(ws_switch):
    """VERDICT r4 (weak 4) / ADVICE r3: a FINITE fp32 operand above the largest bf16 (3.3895e38 < |x| <= 3.4028e38) used to round
    its first piece to +-Inf and poison every output it touches with NaN; the first piece is now clamped to +-bf16max and the
    split stays exact.  Checked on the activation operand (in-loop split, both kernels) and on the weight operand (pre-split
    planes), forward, data gradient and weight gradient, against float64."""
    Kn = ws_switch
    Kn.CONV_ALGO.update(wino=0)
    torch.manual_seed(4)
    big = 3.4e38
    for on, Cin in ((True, 128), (False, 128), (True, 64)):      # Cin 128: k_wgrad_tr; 64: conv.hip's weight-gradient kernel
        Kn.CONV_WS["on"] = on
        conv = Kn.Conv2d(Cin, 128, 1, bias=False).to(DEV)
        with torch.no_grad():
            conv.weight.mul_(1e-3)
        x = (torch.randn(2, Cin, 9, 9, device=DEV) * 1e-2).contiguous(memory_format=CL)
        xx = x.clone()
        xx[0, 5, 3, 4] = big
        xx[1, 7, 0, 0] = -big
        xx.requires_grad_(True)
        y = conv(xx)
        gy = (torch.randn_like(y) * 1e-3).contiguous(memory_format=CL)
        gy[0, 3, 2, 2] = big * 1e-3        # a large (finite) gradient entry: data and weight gradient operands
        conv.weight.grad = None
        y.backward(gy)
        torch.cuda.synchronize()
        assert torch.isfinite(y).all() and torch.isfinite(xx.grad).all() and torch.isfinite(conv.weight.grad).all()
        w64 = conv.weight.detach().double().reshape(128, Cin)
        ref = torch.einsum("nchw,oc->nohw", xx.detach().double(), w64)
        assert float((y.double() - ref).abs().max() / ref.abs().max()) < 1e-6
        dref = torch.einsum("nohw,oc->nchw", gy.double(), w64)
        assert float((xx.grad.double() - dref).abs().max() / dref.abs().max()) < 1e-6
        wref = torch.einsum("nohw,nchw->oc", gy.double(), xx.detach().double())
        assert float((conv.weight.grad.double().reshape(128, Cin) - wref).abs().max() / wref.abs().max()) < 1e-6
        # the weight operand
        with torch.no_grad():
            w0 = conv.weight[7, 9, 0, 0].item()
            conv.weight[7, 9, 0, 0] = big
            y2 = conv(x)
            conv.weight[7, 9, 0, 0] = w0
        torch.cuda.synchronize()
        assert torch.isfinite(y2).all() and float(y2[:, 7].abs().max()) > 1e30


# ---------------------------------------------------------------------------------------------------------------------------
# split-fp16 (round 6): three fp16 piece products per fp32 product, operands scaled per tensor by a power of two taken from the
# maxima their producers leave (csrc/conv_geom.h).  Not the bits of the six-product form -- an independent arithmetic of the same
# class: checked against float64 (never worse than the six-product form by more than 25 %), against itself across tile plans,
# and its plumbing (fused maxima == the tensor's max |x|, stale maxima are never used, batched plane rebuilds == lazy ones).
# ---------------------------------------------------------------------------------------------------------------------------
def _conv64(x, w, stride, pad, dil, gy):
    import torch.nn.functional as F
    xd = x.detach().cpu().double().contiguous().requires_grad_(True)
    wd = w.detach().cpu().double().contiguous().requires_grad_(True)
    y = F.conv2d(xd, wd, stride=stride, padding=pad, dilation=dil)
    y.backward(gy.detach().cpu().double().contiguous())
    return y.detach(), xd.grad, wd.grad


def _run_h(Kn, h, conv, x, gy, pivot=None):
    Kn.CONV_H["on"] = h
    Kn.CONV_WS["on"] = True
    xx = x.detach().clone().requires_grad_(True)
    conv.weight.grad = None
    if pivot is None:
        y, sums = conv(xx), None
    else:
        y, sums = conv(xx, stat_pivot=pivot)
        sums = Kn.finished_sums(sums, conv.out_channels)
    y.backward(gy)
    torch.cuda.synchronize()
    return y.detach(), xx.grad.detach(), conv.weight.grad.detach().clone(), sums


@pytest.mark.parametrize("Cin,Cout,k,stride,dil,H,W,N,bias", CASES)
def test_wsh_forward_dgrad_wgrad_stats_against_float64(Cin, Cout, k, stride, dil, H, W, N, bias, wsh_switch):
    Kn = wsh_switch
    Kn.CONV_ALGO.update(wino=0)
    torch.manual_seed(Cin * 7 + Cout + k + dil)
    conv = Kn.Conv2d(Cin, Cout, k, stride=stride, padding=dil * (k // 2), dilation=dil, bias=bias).to(DEV)
    # post-ReLU-like activations and a gradient whose rows span six decades (what the loss heads hand back)
    x = torch.relu(torch.randn(N, Cin, H, W, device=DEV) + 0.3).contiguous(memory_format=CL)
    Ho = (H + 2 * dil * (k // 2) - dil * (k - 1) - 1) // stride + 1
    Wo = (W + 2 * dil * (k // 2) - dil * (k - 1) - 1) // stride + 1
    gy = (torch.randn(N, Cout, Ho, Wo, device=DEV) * 1e-4 * 10.0 ** (-6 * torch.rand(N, 1, Ho, Wo, device=DEV))).contiguous(memory_format=CL)
    pivot = torch.randn(Cout, device=DEV) * 0.1
    ref = _conv64(x, conv.weight, stride, dil * (k // 2), dil, gy)
    if bias:
        ref = (ref[0] + conv.bias.detach().cpu().double().view(1, -1, 1, 1),) + ref[1:]
    got = {h: _run_h(Kn, h, conv, x, gy) for h in (False, True)}
    for i, name in enumerate(("y", "dx", "dw")):
        sc = ref[i].abs().max()
        e6 = float((got[False][i].cpu().double() - ref[i]).abs().max() / sc)
        e3 = float((got[True][i].cpu().double() - ref[i]).abs().max() / sc)
        assert e3 <= 1.25 * e6 + 2e-7, (name, e3, e6)
        assert e3 < 3e-6, (name, e3)
    # ... and element-wise: a pixel whose dx is wrong relative to ITSELF fails here even when the max-normalised error passes
    bnd = SB.conv_refs(x, conv.weight, gy, stride, dil * (k // 2), dil)
    if bias:
        bnd["y"] = (bnd["y"][0], bnd["y"][1] + SB.EPS * ref[0].abs())
    for i, name in enumerate(("y", "dx", "dw")):
        e = SB.excess(got[True][i], ref[i], bnd[name][1])
        assert e <= 1.0, (name, e)
    # the fused BatchNorm statistics describe THIS arithmetic's output: equal to the stand-alone statistics pass over it to fp32
    # rounding of the column sums (both are pivot-shifted sums of the same values, added in different orders)
    ys, _, _, sums = _run_h(Kn, True, conv, x, gy, pivot)
    assert torch.equal(ys, got[True][0])
    if Cout % 4:
        return          # (the stand-alone statistics pass reads float4 columns)
    from u2pl_amd._lib import call, query
    rows, ld = Kn.as_rows(ys)
    M = ys.shape[0] * ys.shape[2] * ys.shape[3]
    alone = torch.empty(2 * Cout + 1, dtype=torch.float64, device=DEV)
    wsb = torch.empty(query("u2pl_colreduce_workspace_bytes", M, 1, Cout), dtype=torch.uint8, device=DEV)
    call("u2pl_bn_stats_f32", rows, ld, M, Cout, pivot, wsb, alone)
    torch.cuda.synchronize()
    tol = 1e-5 * (alone[: 2 * Cout].abs().max() + 1)
    assert float((sums[: 2 * Cout] - alone[: 2 * Cout]).abs().max()) <= float(tol)


@pytest.mark.parametrize("Cin,Cout,k,stride,dil,H,W,N,bias", [c for c in CASES if c[0] * c[2] * c[2] >= 128][:10])
def test_wsh_same_bits_across_tile_plans(Cin, Cout, k, stride, dil, H, W, N, bias, wsh_switch):
    """persistent blocks walking (tile, chunk) streams == one block per tile: the plan changes which block computes a tile and
    in which LDS stage, never the order of a tile's products"""
    from u2pl_amd._lib import query
    Kn = wsh_switch
    Kn.CONV_ALGO.update(wino=0)
    torch.manual_seed(3 + Cin + Cout)
    conv = Kn.Conv2d(Cin, Cout, k, stride=stride, padding=dil * (k // 2), dilation=dil, bias=bias).to(DEV)
    x = torch.randn(N, Cin, H, W, device=DEV).contiguous(memory_format=CL)
    Ho = (H + 2 * dil * (k // 2) - dil * (k - 1) - 1) // stride + 1
    Wo = (W + 2 * dil * (k // 2) - dil * (k - 1) - 1) // stride + 1
    gy = torch.randn(N, Cout, Ho, Wo, device=DEV).contiguous(memory_format=CL)
    outs = []
    old = query("u2pl_igemm_ws_set_persist", 1)
    try:
        for persist in (1, 0):
            query("u2pl_igemm_ws_set_persist", persist)
            outs.append(_run_h(Kn, True, conv, x, gy, torch.zeros(Cout, device=DEV)))
    finally:
        query("u2pl_igemm_ws_set_persist", old)
    for a, b in zip(outs[0][:3], outs[1][:3]):
        assert torch.equal(a, b)
    assert torch.equal(outs[0][3][: 2 * Cout], outs[1][3][: 2 * Cout])          # (slot 2C, the row count, is the BatchNorm's to fill)


# The smallest pointwise forward that runs under all four plans: 257 wide tiles (one round + 1; mixing needs a full round), Cout = 256, and
# the first reduction length at which the model still mixes when the plan costs two launches (U2PL_WS_MIX2 = 1: 8 fixed units instead of
# 2; 1.575 n + 14 < 1.725 n + 6 chunks for the six-product planes, 1.575 n + 28 < 1.725 n + 12 for split-fp16 with U2PL_WS_FIX2 = 2:
# n = 54 and 107 chunks of 32).  In one launch the mixed plan wins from 14 and 27 chunks on (tests/test_ws_plan_cpu.py).  (np, Cin):
PLAN_BITS = ((3, 1728), (2, 3424))
PLAN_ROWS, PLAN_COUT = 257 * 128, 256


def _plan_bits_outputs():
    """the pointwise forward with fused statistics of PLAN_BITS under this process's switches -> [(plan, y, 2 Cout sums)] (CPU tensors)"""
    Kn = K()
    Kn.CONV_ALGO.update(wino=0)
    Kn.CONV_WS["on"] = True
    out = []
    for np_, Cin in PLAN_BITS:
        Kn.CONV_H["on"] = np_ == 2
        # the call must reach k_igemm_ws, or the plans compared are no plans: the pre-split route on, no bf16-operand student
        assert Kn._ws_ok(PLAN_COUT, Cin) and not Kn.CONV_ALGO.get("bf16", 0), (dict(Kn.CONV_ALGO), dict(Kn.CONV_WS))
        g = torch.Generator().manual_seed(100 + Cin)
        conv = Kn.Conv2d(Cin, PLAN_COUT, 1, bias=True)
        with torch.no_grad():
            conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) / Cin ** 0.5)
            conv.bias.copy_(torch.randn(PLAN_COUT, generator=g))
        conv = conv.to(DEV)
        gd = torch.Generator(device=DEV).manual_seed(200 + Cin)       # (the same seeded device generator in every process: the same x)
        x = torch.randn(1, 257, 128, Cin, device=DEV, generator=gd).permute(0, 3, 1, 2)
        pivot = (torch.randn(PLAN_COUT, generator=g) * 0.1).to(DEV)
        y, sums = conv(x, stat_pivot=pivot)
        sums = Kn.finished_sums(sums, PLAN_COUT)
        torch.cuda.synchronize()
        out.append((_ws_plan(PLAN_ROWS, Cin, PLAN_COUT, 1, np_), y.detach().cpu(), sums.detach()[: 2 * PLAN_COUT].cpu()))
    return out


@pytest.fixture(scope="module")
def plan_bits_default():
    """the outputs under this process's own (default) plan, computed once for the forced plans to be compared with"""
    assert not any(os.environ.get(v) for v in WS_PLAN_SWITCHES), "run the suite without the tile-plan switches: this test sets each itself"
    saved = (dict(K().CONV_ALGO), dict(K().CONV_WS), dict(K().CONV_H))
    try:
        return _plan_bits_outputs()
    finally:
        for d, s_ in zip((K().CONV_ALGO, K().CONV_WS, K().CONV_H), saved):
            d.update(s_)


@pytest.mark.parametrize("name,value,plan", [("U2PL_WS_NARROW", "0", (0, 257, 0)), ("U2PL_WS_NARROW", "1", (1, 0, 514)), ("U2PL_WS_MIX2", "1", (3, 256, 2))])
def test_same_bits_under_the_wide_narrow_mixed_and_two_launch_plans(name, value, plan, plan_bits_default, tmp_path):
    """INTEGRATION.md promises "Same bits" for U2PL_WS_NARROW and U2PL_WS_MIX2: a tile plan changes which block computes a tile, never the
    order of a tile's products or of its statistics rows.  The switches are read once per process: the default (mixed, asserted through the
    query) runs here, the forced plan in one child of this file, which is ended at its time limit; y and the 2 Cout statistics sums must
    agree bit for bit."""
    import subprocess
    mine = plan_bits_default
    assert [o[0] for o in mine] == [(2, 256, 2), (2, 256, 2)]                 # mixed: 256 wide tiles + the 257th as two narrow ones
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = str(tmp_path / "forced.pt")
    env = dict(os.environ, PYTHONPATH=root)
    env[name] = value
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path], cwd=root, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (name, value, r.stderr[-2000:])
    for (np_, Cin), a, b in zip(PLAN_BITS, mine, torch.load(path)):
        assert tuple(b[0]) == plan, (name, value, np_, b[0])
        assert torch.equal(a[1], b[1]), (name, value, np_, "y differs", float((a[1] - b[1]).abs().max()))
        assert torch.equal(a[2], b[2]), (name, value, np_, "statistics differ")


@pytest.mark.parametrize("Cin,Cout,dil,H,W,N", [(256, 256, 2, 33, 29, 2), (512, 512, 4, 21, 21, 1), (128, 128, 1, 37, 37, 1)])
def test_wsh_winograd_layers_against_float64(Cin, Cout, dil, H, W, N, wsh_switch):
    from u2pl_amd._lib import query
    Kn = wsh_switch
    Kn.CONV_ALGO.update(wino=4, min_gain=0.0)
    torch.manual_seed(Cin + Cout + dil)
    conv = Kn.Conv2d(Cin, Cout, 3, padding=dil, dilation=dil, bias=False).to(DEV)
    x = torch.relu(torch.randn(N, Cin, H, W, device=DEV)).contiguous(memory_format=CL)
    gy = (torch.randn(N, Cout, H, W, device=DEV) * 1e-5).contiguous(memory_format=CL)
    ref = _conv64(x, conv.weight, 1, dil, dil, gy)
    got = {h: _run_h(Kn, h, conv, x, gy) for h in (False, True)}
    for i, name in enumerate(("y", "dx", "dw")):
        sc = ref[i].abs().max()
        e6 = float((got[False][i].cpu().double() - ref[i]).abs().max() / sc)
        e3 = float((got[True][i].cpu().double() - ref[i]).abs().max() / sc)
        assert e3 <= 1.25 * e6 + 2e-7, (name, e3, e6)        # (the Winograd transforms dominate both: ~1e-5)
    # element-wise, through the transforms (tests/split_bounds.py: F(4x4) restated from csrc/wino.hip)
    nsplit = query("u2pl_wgrad_batched_splits", query("u2pl_wino_tiles", N, H, W, dil, 4), Cin, Cout, 36)
    bounds = (SB.wino_conv(x, conv.weight, dil, 4), SB.wino_conv(gy, conv.weight.detach().flip(2, 3).transpose(0, 1), dil, 4),
              SB.wino_wgrad(x, gy, dil, 4, nsplit))
    for i, name in enumerate(("y", "dx", "dw")):
        e = SB.excess(got[True][i], bounds[i][0], bounds[i][1])
        assert e <= 1.0, (name, e)


def test_fused_operand_maxima_equal_the_tensors_maxima(wsh_switch):
    """BatchNorm apply / backward apply and the Winograd transforms leave max |output| in an amax object as they write; the
    stand-alone pass gives the same value; NaN anywhere makes the maximum NaN"""
    from u2pl_amd._lib import call, query
    Kn = wsh_switch
    torch.manual_seed(9)
    nw = query("u2pl_amax_words")

    def value(obj):
        return obj.view(torch.int32).max().view(torch.float32)

    bn = Kn.BatchNorm2d(96).to(DEV).train()
    x = torch.randn(3, 96, 23, 17, device=DEV).contiguous(memory_format=CL).requires_grad_(True)
    res = torch.randn(3, 96, 23, 17, device=DEV).contiguous(memory_format=CL).requires_grad_(True)
    y = bn(x, res=res, relu=True)
    obj, ver = y._u2pl_amax
    assert obj.numel() == nw and ver == y._version
    assert float(value(obj)) == float(y.detach().abs().max())
    gy = (torch.randn_like(y) * 1e-3).contiguous(memory_format=CL)
    gx, gres = torch.autograd.grad(y, (x, res), gy)
    assert float(value(gx._u2pl_amax[0])) == float(gx.abs().max())
    assert float(value(gres._u2pl_amax[0])) == float(gres.abs().max())
    # stand-alone pass; a torch in-place op invalidates a carried maximum
    t = torch.randn(2, 64, 9, 9, device=DEV).contiguous(memory_format=CL)
    a = Kn.amax_of(t)
    assert float(value(a)) == float(t.abs().max())
    assert Kn.amax_of(t) is a                       # cached for this version of the tensor
    t.mul_(3.0)
    b = Kn.amax_of(t)
    assert b is not a and float(value(b)) == float(t.abs().max())
    t[1, 3, 2, 2] = float("nan")
    assert torch.isnan(value(Kn.amax_of(t)))
    # Winograd input transform
    tiles = query("u2pl_wino_tiles", 2, 9, 9, 1, 4)
    V = torch.empty(36 * tiles * 64, device=DEV)
    slot = Kn.amax_slot(t.device)
    t2 = torch.randn(2, 64, 9, 9, device=DEV).contiguous(memory_format=CL)
    call("u2pl_wino_input_amax_f32", t2, 64, 2, 9, 9, 64, 1, 4, V, slot)
    assert float(value(slot)) == float(V.abs().max())
    Mg = torch.empty(36 * tiles * 64, device=DEV)
    slot2 = Kn.amax_slot(t.device)
    call("u2pl_wino_gy_amax_f32", t2, 64, 2, 9, 9, 64, 1, 4, Mg, slot2)
    assert float(value(slot2)) == float(Mg.abs().max())


@pytest.mark.parametrize("k,Cout,H", [(1, 384, 27), (1, 256, 140), (3, 256, 33)])
def test_eval_epilogue_leaves_the_outputs_maximum(k, Cout, H, wsh_switch):
    """conv + eval-mode BatchNorm in one launch (GEMM epilogue / Winograd output transform): the amax object holds max |y| of what
    was STORED -- rows past M and columns past Cout of the last tiles do not count (persistent blocks, several tiles per block at
    H = 140)"""
    Kn = wsh_switch
    Kn.CONV_ALGO.update(wino=4 if k == 3 else 0, min_gain=0.0)
    torch.manual_seed(6 + k)
    conv = Kn.Conv2d(256, Cout, k, padding=k // 2, bias=False).to(DEV)
    bn = Kn.BatchNorm2d(Cout).to(DEV).eval()
    with torch.no_grad():
        bn.running_mean.normal_(0, 0.2)
        bn.running_var.uniform_(0.5, 2.0)
        bn.bias.normal_(0, 5.0)             # (a large shift: a zero-filled padding row would read |beta|, not 0)
        x = torch.randn(2, 256, H, H - 4, device=DEV).contiguous(memory_format=CL)
        y = Kn.conv_bn_eval(conv, bn, x, relu=False)
    obj, ver = y._u2pl_amax
    assert ver == y._version
    assert float(obj.view(torch.int32).max().view(torch.float32)) == float(y.abs().max())


def test_wsh_eval_batchnorm_epilogue_has_the_two_kernel_forms_bits(wsh_switch):
    Kn = wsh_switch
    Kn.CONV_ALGO.update(wino=0)
    torch.manual_seed(5)
    conv = Kn.Conv2d(256, 384, 1, bias=False).to(DEV)
    bn = Kn.BatchNorm2d(384).to(DEV).eval()
    with torch.no_grad():
        bn.running_mean.normal_(0, 0.2)
        bn.running_var.uniform_(0.5, 2.0)
        bn.weight.normal_(1.0, 0.2)
        bn.bias.normal_(0, 0.2)
        x = torch.randn(2, 256, 27, 23, device=DEV).contiguous(memory_format=CL)
        r = torch.randn(2, 384, 27, 23, device=DEV).contiguous(memory_format=CL)
        fused = Kn.conv_bn_eval(conv, bn, x, res=r, relu=True)
        two = bn(conv(x), res=r, relu=True)
    torch.cuda.synchronize()
    assert torch.equal(fused, two)


def test_wsh_presplit_planes_equal_the_lazy_paths(wsh_switch):
    """fp16 planes + per-matrix maxima: the batched rebuild after an optimizer step (clear + maxima + split: three launches, plus
    the Winograd filter transform) writes the bytes the per-weight lazy path writes"""
    from u2pl_amd._lib import query
    Kn = wsh_switch
    Kn.CONV_ALGO.update(wino=4, min_gain=0.0)
    saved = Kn.PRESPLIT["on"]
    torch.manual_seed(21)
    convs = [Kn.Conv2d(128, 256, 1, bias=False).to(DEV), Kn.Conv2d(256, 128, 3, padding=2, dilation=2, bias=False).to(DEV),
             Kn.Conv2d(128, 160, 3, stride=2, padding=1, bias=False).to(DEV), Kn.Conv2d(160, 96, 1, bias=True).to(DEV)]
    arena = Kn.ParamArena([[p for c in convs for p in c.parameters()]])
    x = torch.randn(2, 128, 21, 19, device=DEV).contiguous(memory_format=CL)

    def step():
        h = x.clone().requires_grad_(True)
        y = h
        for c in convs:
            y = c(y)
        y.square().mean().backward()
        torch.cuda.synchronize()
        return y.detach().clone(), h.grad.clone()

    try:
        Kn.PRESPLIT["on"] = False
        step()
        kinds = sorted(k for c in convs for k in c.weight._u2pl_derived)
        assert kinds == sorted(["fh", "dh", "wf4h", "wd4h", "fh", "dh", "fh", "dh"]), kinds
        arena.grad.normal_(0, 1.0)
        arena.sgd_step([0.05], 0.9, 1e-4)
        y_lazy, dx_lazy = step()
        lazy = {(i, k): e["buf"].clone() for i, c in enumerate(convs) for k, e in c.weight._u2pl_derived.items()}
        Kn.PRESPLIT["on"] = True
        for c in convs:
            for e in c.weight._u2pl_derived.values():
                e["buf"].zero_()
        Kn.bump_weight_epoch()
        k0 = query("u2pl_kernel_launches")
        n = Kn.presplit(arena.params, arena)
        assert n == 8 and query("u2pl_kernel_launches") - k0 == 4
        torch.cuda.synchronize()
        for (i, k), b in lazy.items():
            e = convs[i].weight._u2pl_derived[k]
            assert torch.equal(e["buf"], b), (i, k)
        y_pre, dx_pre = step()
        assert torch.equal(y_pre, y_lazy) and torch.equal(dx_pre, dx_lazy)
    finally:
        Kn.PRESPLIT["on"] = saved


def test_wsh_operand_range_semantics(wsh_switch):
    """what the per-tensor power-of-two scale promises: finite operands of any magnitude (1e-30 .. 3e38)
    give finite, accurate results; an element 2^-16 of the tensor's maximum or larger keeps fp32 accuracy; smaller elements are
    carried with an ABSOLUTE error of 2^-40 of the maximum; NaN / Inf operands give non-finite outputs in the rows they touch"""
    Kn = wsh_switch
    Kn.CONV_ALGO.update(wino=0)
    torch.manual_seed(4)
    conv = Kn.Conv2d(128, 128, 1, bias=False).to(DEV)
    w64 = conv.weight.detach().double().reshape(128, 128)
    for scale in (1e-30, 1.0, 1e30):
        x = (torch.randn(2, 128, 9, 9, device=DEV) * scale).contiguous(memory_format=CL).requires_grad_(True)
        y = conv(x)
        gy = (torch.randn_like(y) * (1e-6 / scale if scale > 1 else 1e-6)).contiguous(memory_format=CL)
        conv.weight.grad = None
        y.backward(gy)
        torch.cuda.synchronize()
        ref = torch.einsum("nchw,oc->nohw", x.detach().double(), w64)
        assert float((y.double() - ref).abs().max() / ref.abs().max()) < 1e-6
        dref = torch.einsum("nohw,oc->nchw", gy.double(), w64)
        assert float((x.grad.double() - dref).abs().max() / dref.abs().max()) < 1e-6
        wref = torch.einsum("nohw,nchw->oc", gy.double(), x.detach().double())
        assert float((conv.weight.grad.double().reshape(128, 128) - wref).abs().max() / wref.abs().max()) < 1e-6
    # one huge finite element: the others keep an absolute error of 2^-40 of it per term
    x = torch.randn(2, 128, 9, 9, device=DEV).contiguous(memory_format=CL)
    x[0, 5, 3, 4] = 3.0e38
    with torch.no_grad():
        y = conv(x)
    assert torch.isfinite(y).all()
    ref = torch.einsum("nchw,oc->nohw", x.double(), w64)
    cond = torch.einsum("nchw,oc->nohw", x.double().abs(), w64.abs())
    bound = 128 * 2.0 ** -39 * 3.0e38 * float(w64.abs().max()) + 2.0 ** -22 * cond          # the floor + the usual relative term
    assert bool(((y.double() - ref).abs() <= bound).all())
    # non-finite operands
    x = torch.randn(2, 128, 9, 9, device=DEV).contiguous(memory_format=CL)
    x[1, 7, 2, 2] = float("nan")
    with torch.no_grad():
        y = conv(x)
    assert not torch.isfinite(y[1, :, 2, 2]).any()


@pytest.mark.parametrize("Cin,Cout,k,dil,wino", [(1024, 256, 1, 1, 0), (256, 1024, 1, 1, 0), (256, 256, 3, 2, 4), (2048, 256, 3, 12, 0)])
def test_wsh_power_of_two_homogeneity_is_exact_at_the_headline_sizes(Cin, Cout, k, dil, wino, wsh_switch):
    """A size-independent property of the per-tensor power-of-two scaling, checked BIT-EXACTLY on layer3 / ASPP shapes of the 769^2
    step (4 x 97^2 pixels): multiplying the activations by 2^a, the weights by 2^c and the incoming gradient by 2^b presents the
    matrix cores with the very same scaled fp16 pieces, so y, dx, dw and the fused BatchNorm sums come back multiplied by exactly
    2^(a+c), 2^(b+c), 2^(a+b) and 2^(a+c) / 2^(2(a+c)) -- through the direct kernels and through the Winograd transforms alike."""
    Kn = wsh_switch
    Kn.CONV_ALGO.update(wino=wino, min_gain=0.0)
    torch.manual_seed(Cin + Cout + k)
    N, H = 4, 97
    conv = Kn.Conv2d(Cin, Cout, k, padding=dil * (k // 2), dilation=dil, bias=False).to(DEV)
    x = torch.relu(torch.randn(N, Cin, H, H, device=DEV) + 0.2).contiguous(memory_format=CL)
    gy = (torch.randn(N, Cout, H, H, device=DEV) * 1e-4).contiguous(memory_format=CL)
    pivot = torch.randn(Cout, device=DEV) * 0.1
    y0, dx0, dw0, s0 = _run_h(Kn, True, conv, x, gy, pivot)
    a, b, c = 7, -5, 3
    with torch.no_grad():
        conv.weight.mul_(2.0 ** c)
    y1, dx1, dw1, s1 = _run_h(Kn, True, conv, (x * 2.0 ** a).contiguous(memory_format=CL), (gy * 2.0 ** b).contiguous(memory_format=CL),
                              pivot * 2.0 ** (a + c))
    assert torch.equal(y1, y0 * 2.0 ** (a + c))
    assert torch.equal(dx1, dx0 * 2.0 ** (b + c))
    assert torch.equal(dw1, dw0 * 2.0 ** (a + b))
    assert torch.equal(s1[:Cout], s0[:Cout] * 2.0 ** (a + c))
    assert torch.equal(s1[Cout:2 * Cout], s0[Cout:2 * Cout] * 4.0 ** (a + c))


if __name__ == "__main__":          # a child of test_same_bits_under_the_wide_narrow_mixed_and_two_launch_plans: argv[1] = where to save
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    torch.save(_plan_bits_outputs(), sys.argv[1])
