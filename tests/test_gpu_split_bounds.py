"""-m gpu: every route by which a product reaches the split-fp16 kernels (U2PL_CONV_H=1, the default), held ELEMENT-WISE to the
float64 bound of INTEGRATION.md section 4 (tests/split_bounds.py: a fp32-class term in units of eps32 * sum |a||b| plus the
documented floor of 2^-40 of each operand's maximum, carried through the Winograd transforms and the epilogues), and the maximum
contract checked at every split-fp16 launch of real training / evaluation steps.

Routes (the dispatch branches of u2pl_amd/nn.py):
  forward        u2pl_conv2d_fwd_wsh_f32, ..._fwd_bnstats_wsh_f32 (fused statistics), ..._fwd_bnact_wsh_f32 (eval BatchNorm +
                 residual + ReLU), Winograd F(4) / F(2) through u2pl_gemm_batched_wsh_f32 with the plain and the BN-act output
  data gradient  u2pl_conv2d_dgrad_wsh_f32, the pointwise data gradient through ..._fwd_bnact_wsh_f32 with the GradJoin running
                 sum as its residual, Winograd transposed with and without the join epilogue
  weight grad    u2pl_conv2d_wgrad_h_f32 (accumulate 0 and 1), u2pl_wgrad_batched_h_f32 + u2pl_wino_wgrad_finish_f32"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import split_bounds as SB  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
CL = torch.channels_last

H_ENTRIES = ("u2pl_conv2d_fwd_wsh_f32", "u2pl_conv2d_fwd_bnstats_wsh_f32", "u2pl_conv2d_fwd_bnact_wsh_f32", "u2pl_conv2d_dgrad_wsh_f32",
             "u2pl_gemm_batched_wsh_f32", "u2pl_conv2d_wgrad_h_f32", "u2pl_wgrad_batched_h_f32")


@pytest.fixture
def Kn(monkeypatch):
    """split-fp16 on, pre-split weights on; every switch restored afterwards; a recorder of the entry points each test reaches"""
    from u2pl_amd import nn as K
    saved = (dict(K.CONV_ALGO), dict(K.CONV_WS), dict(K.CONV_H))
    K.CONV_H["on"] = True
    K.CONV_WS["on"] = True
    with SB.recorded_calls(K) as seen:
        monkeypatch.setattr(K, "_seen", seen, raising=False)
        yield K
    K.CONV_ALGO.update(saved[0])
    K.CONV_WS.update(saved[1])
    K.CONV_H.update(saved[2])


def _operands(kind, N, Cin, Cout, k, H, W, Ho, Wo, g):
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) / (k * k * Cin) ** 0.5
    gy = torch.randn(N, Cout, Ho, Wo, generator=g)
    if kind == "relu_heavy_tail":
        x = torch.relu(x - 0.25) ** 3
        gy = gy * (torch.rand(gy.shape, generator=g) < 0.3)
    elif kind == "six_decade_rows":
        x = torch.relu(x + 0.3)
        gy = gy * 1e-4 * 10.0 ** (-6 * torch.rand(N, 1, Ho, Wo, generator=g))
    elif kind == "twelve_decades":
        sc = 10.0 ** (torch.rand(Cin, generator=g) * 12 - 6)
        x = x * sc.view(1, Cin, 1, 1)
        w = w / sc.view(1, Cin, 1, 1)
    elif kind == "cancellation":
        base = torch.randn(N, Cin // 2, H, W, generator=g)
        x = torch.stack((base, base * (1 + 1e-4 * torch.randn(base.shape, generator=g))), 2).reshape(N, Cin, H, W)
        wh = torch.randn(Cout, Cin // 2, k, k, generator=g) / (k * k * Cin) ** 0.5
        w = torch.stack((wh, -wh), 2).reshape(Cout, Cin, k, k)
    else:
        raise ValueError(kind)
    return x, w, gy


def _conv(Kn, Cin, Cout, k, stride, dil, bias, w, b=None):
    conv = Kn.Conv2d(Cin, Cout, k, stride=stride, padding=dil * (k // 2), dilation=dil, bias=bias).to(DEV)
    with torch.no_grad():
        conv.weight.copy_(w.to(DEV))
        if bias:
            conv.bias.copy_(b.to(DEV))
    return conv


def _run(conv, x, gy, pivot=None):
    xx = x.to(DEV).contiguous(memory_format=CL).requires_grad_(True)
    conv.weight.grad = None
    out = conv(xx) if pivot is None else conv(xx, stat_pivot=pivot)[0]
    out.backward(gy.to(DEV).contiguous(memory_format=CL))
    torch.cuda.synchronize()
    return out.detach(), xx.grad.detach(), conv.weight.grad.detach().clone()


def _held(name, got, ref, bound):
    e = SB.excess(got, ref, bound)
    assert e <= 1.0, f"{name}: error {e:.3g}x the element-wise bound"
    return e


def _geom(H, W, k, stride, dil):
    pad = dil * (k // 2)
    return (H + 2 * pad - dil * (k - 1) - 1) // stride + 1, (W + 2 * pad - dil * (k - 1) - 1) // stride + 1


# ---- direct (implicit-GEMM) routes: forward, fused statistics, data gradient, weight gradient -----------------------------------
def _cases():
    from test_gpu_igemm_ws import CASES
    return CASES


@pytest.mark.parametrize("kind", ["relu_heavy_tail", "twelve_decades", "cancellation"])
@pytest.mark.parametrize("Cin,Cout,k,stride,dil,H,W,N,bias", _cases())
def test_direct_routes_meet_the_element_wise_bound(Cin, Cout, k, stride, dil, H, W, N, bias, kind, Kn):
    """y (u2pl_conv2d_fwd_wsh_f32 and, with a statistics pivot, ..._bnstats_wsh_f32), dx (u2pl_conv2d_dgrad_wsh_f32) and dw
    (u2pl_conv2d_wgrad_h_f32 where Cin, Cout >= 128) on the layer table of test_gpu_igemm_ws.py: Cout % 4 != 0, ragged maps, a
    dilation halo larger than the map, filter-row skipping and the mixed tile plan included.  (The six-decade gradient rows are
    test_wsh_forward_dgrad_wgrad_stats_against_float64's operands.)"""
    Kn.CONV_ALGO.update(wino=0)
    g = torch.Generator().manual_seed(Cin * 7 + Cout + k + dil + len(kind))
    Ho, Wo = _geom(H, W, k, stride, dil)
    x, w, gy = _operands(kind, N, Cin, Cout, k, H, W, Ho, Wo, g)
    b = torch.randn(Cout, generator=g) * 0.1 if bias else None
    conv = _conv(Kn, Cin, Cout, k, stride, dil, bias, w, b)
    y, dx, dw = _run(conv, x, gy)
    ys, _, _ = _run(conv, x, gy, pivot=torch.randn(Cout, device=DEV) * 0.1)
    ref = SB.conv_refs(x, w, gy, stride, dil * (k // 2), dil)
    ry, by = ref["y"]
    if bias:       # the epilogue's bias add: one fp32 rounding of the output
        ry = ry + b.double().view(1, -1, 1, 1)
        by = by + SB.EPS * ry.abs()
    _held("y", y, ry, by)
    _held("y (fused statistics)", ys, ry, by)
    _held("dx", dx, *ref["dx"])
    _held("dw", dw.reshape(ref["dw"][0].shape), *ref["dw"])
    assert Kn._seen.get("u2pl_conv2d_fwd_wsh_f32") and Kn._seen.get("u2pl_conv2d_fwd_bnstats_wsh_f32")
    if Cin > 64 and Cout % 32 == 0:
        assert Kn._seen.get("u2pl_conv2d_dgrad_wsh_f32")
    if min(Cin, Cout) >= 128 and Cout % 32 == 0:
        assert Kn._seen.get("u2pl_conv2d_wgrad_h_f32")


def test_weight_gradient_accumulate_into_the_arena_sink(Kn):
    """u2pl_conv2d_wgrad_h_f32 with accumulate = 1 (the arena's gradient sink already holds a contribution) and the Winograd-domain
    finish with accumulate = 1: sink = previous + dw, held to the bound plus one fp32 rounding of the sum"""
    g = torch.Generator().manual_seed(31)
    for k, wino in ((1, 0), (3, 0), (3, 4)):
        Kn.CONV_ALGO.update(wino=wino, min_gain=0.0)
        Cin, Cout, H, W, N = 256, 128, 19, 23, 2
        x, w, gy = _operands("six_decade_rows", N, Cin, Cout, k, H, W, H, W, g)
        conv = _conv(Kn, Cin, Cout, k, 1, 1, False, w)
        arena = Kn.ParamArena([[conv.weight]])
        Kn._seen.clear()
        # the sink's previous contribution at the size of dw itself: an overwrite instead of an add misses by ~|dw|
        scale = float(SB.conv_dw_bound(gy, x, (k, k), 1, k // 2, 1)[0].abs().mean())
        arena.grad.copy_((torch.randn(arena.grad.shape, generator=g) * scale).to(DEV))
        pv = conv.weight._u2pl_grad.detach().cpu().double().clone()
        xx = x.to(DEV).contiguous(memory_format=CL).requires_grad_(True)
        conv(xx).backward(gy.to(DEV).contiguous(memory_format=CL))
        Kn.wgrad_stream_sync()
        torch.cuda.synchronize()
        got = conv.weight._u2pl_grad.detach().cpu().double()
        if wino:
            nsplit = Kn.query("u2pl_wgrad_batched_splits", Kn.query("u2pl_wino_tiles", N, H, W, 1, wino), Cin, Cout, (wino + 2) ** 2)
            rdw, bdw = SB.wino_wgrad(x, gy, 1, wino, nsplit)
            assert Kn._seen.get("u2pl_wgrad_batched_h_f32")
            assert [c[5] for c in Kn._seen["u2pl_wino_wgrad_finish_f32"]] == [1]          # accumulate argument
        else:
            rdw, bdw = SB.conv_refs(x, w, gy, 1, k // 2, 1)["dw"]
            assert [c[8] for c in Kn._seen["u2pl_conv2d_wgrad_h_f32"]] == [1]             # accumulate argument
        ref = pv + rdw
        _held(f"accumulated dw (k={k}, wino={wino})", got, ref, bdw + SB.EPS * (pv.abs() + rdw.abs()))


# ---- eval-mode BatchNorm epilogue (+ residual + ReLU): direct and Winograd output transform ----------------------------------
@pytest.mark.parametrize("k,wino,Cin,Cout,H,W", [(1, 0, 256, 384, 27, 23), (1, 0, 512, 132, 21, 19), (3, 0, 128, 256, 17, 15),
                                                 (3, 4, 256, 256, 19, 21), (3, 2, 128, 128, 13, 11)])
def test_eval_batchnorm_epilogue_meets_the_bound(k, wino, Cin, Cout, H, W, Kn):
    """conv_bn_eval: u2pl_conv2d_fwd_bnact_wsh_f32 / Winograd with the BN-act output transform, residual and ReLU in the epilogue;
    the GEMM bound scaled by |gamma invstd| plus C_EPI fp32 roundings of the epilogue's terms"""
    Kn.CONV_ALGO.update(wino=wino, min_gain=0.0)
    g = torch.Generator().manual_seed(41 + k + wino + Cout)
    N = 2
    x, w, _ = _operands("relu_heavy_tail", N, Cin, Cout, k, H, W, H, W, g)
    conv = _conv(Kn, Cin, Cout, k, 1, 1, False, w)
    bn = Kn.BatchNorm2d(Cout).to(DEV).eval()
    rm, rv = torch.randn(Cout, generator=g) * 0.2, torch.rand(Cout, generator=g) * 1.5 + 0.5
    gam, bet = torch.randn(Cout, generator=g) * 0.2 + 1.0, torch.randn(Cout, generator=g) * 0.2
    res = torch.randn(N, Cout, H, W, generator=g)
    with torch.no_grad():
        for p, v in ((bn.running_mean, rm), (bn.running_var, rv), (bn.weight, gam), (bn.bias, bet)):
            p.copy_(v.to(DEV))
        y = Kn.conv_bn_eval(conv, bn, x.to(DEV).contiguous(memory_format=CL), res=res.to(DEV).contiguous(memory_format=CL),
                            relu=True)
    torch.cuda.synchronize()
    if wino:
        v, bv = SB.wino_conv(x, w, 1, wino)
        assert Kn._seen.get("u2pl_gemm_batched_wsh_f32")
    else:
        v, bv = SB.conv_refs(x, w, torch.zeros(N, Cout, H, W), 1, k // 2, 1)["y"]
        assert Kn._seen.get("u2pl_conv2d_fwd_bnact_wsh_f32")
    s = (gam.double() / torch.sqrt(rv.double() + bn.eps)).view(1, -1, 1, 1)
    t = bet.double().view(1, -1, 1, 1) - rm.double().view(1, -1, 1, 1) * s
    pre = v * s + t + res.double()
    ref = torch.relu(pre)
    bound = s.abs() * bv + SB.C_EPI * SB.EPS * ((v * s).abs() + (rm.double().view(1, -1, 1, 1) * s).abs()
                                                 + bet.double().abs().view(1, -1, 1, 1) + res.double().abs())
    _held("eval BN epilogue y", y, ref, bound)


# ---- Winograd layers: forward, data gradient (transposed), Winograd-domain weight gradient -----------------------------------
@pytest.mark.parametrize("kind", ["six_decade_rows", "relu_heavy_tail", "twelve_decades", "cancellation"])
@pytest.mark.parametrize("mt", [4, 2])
@pytest.mark.parametrize("Cin,Cout,dil,H,W,N", [(256, 256, 2, 33, 29, 2), (128, 128, 1, 37, 37, 1), (128, 256, 12, 9, 11, 1)])
def test_winograd_routes_meet_the_element_wise_bound(Cin, Cout, dil, H, W, N, mt, kind, Kn):
    """u2pl_gemm_batched_wsh_f32 forward and transposed, u2pl_wgrad_batched_h_f32 + finish: maps that are not a multiple of the tile,
    a dilation halo (12) larger than the map"""
    Kn.CONV_ALGO.update(wino=mt, min_gain=0.0)
    g = torch.Generator().manual_seed(Cin + Cout + dil + mt + len(kind))
    x, w, gy = _operands(kind, N, Cin, Cout, 3, H, W, H, W, g)
    conv = _conv(Kn, Cin, Cout, 3, 1, dil, False, w)
    y, dx, dw = _run(conv, x, gy)
    assert len(Kn._seen.get("u2pl_gemm_batched_wsh_f32", ())) >= 2 and Kn._seen.get("u2pl_wgrad_batched_h_f32")
    _held("winograd y", y, *SB.wino_conv(x, w, dil, mt))
    _held("winograd dx", dx, *SB.wino_conv(gy, w.flip(2, 3).transpose(0, 1), dil, mt))
    nsplit = Kn.query("u2pl_wgrad_batched_splits", Kn.query("u2pl_wino_tiles", N, H, W, dil, mt), Cin, Cout, (mt + 2) ** 2)
    _held("winograd dw", dw, *SB.wino_wgrad(x, gy, dil, mt, nsplit))


# ---- data gradients with the GradJoin running sum folded into the launch ------------------------------------------------------
@pytest.mark.parametrize("k,wino", [(1, 0), (3, 4), (3, 2)])
def test_joined_data_gradient_meets_the_bound(k, wino, Kn):
    """x feeds two convolutions wired to one GradJoin; the one whose backward runs last folds the running sum into its own launch
    (pointwise: u2pl_conv2d_fwd_bnact_wsh_f32 with identity BatchNorm parameters and res = the sum; 3x3: the Winograd transposed
    product's output transform): dx = dx_a + dx_b within both bounds plus one fp32 rounding of the sum"""
    Kn.CONV_ALGO.update(wino=wino, min_gain=0.0)
    g = torch.Generator().manual_seed(51 + k + wino)
    N, C, Ca, Cb, H, W = 2, 128, 256, 192, 17, 19
    x, wa, gya = _operands("six_decade_rows", N, C, Ca, k, H, W, H, W, g)
    _, wb, gyb = _operands("six_decade_rows", N, C, Cb, 1, H, W, H, W, g)
    gyb = gyb * 1e3
    conv_a = _conv(Kn, C, Ca, k, 1, 1, False, wa)      # created first: its backward runs last and takes the join's sum
    conv_b = _conv(Kn, C, Cb, 1, 1, 1, False, wb)
    xx = x.to(DEV).contiguous(memory_format=CL).requires_grad_(True)
    link = Kn.grad_join(xx, 2)
    assert link is not None
    ya = conv_a(xx, grad_link=link)
    yb = conv_b(xx, grad_link=link)
    torch.autograd.backward([ya, yb], [gya.to(DEV).contiguous(memory_format=CL), gyb.to(DEV).contiguous(memory_format=CL)])
    torch.cuda.synchronize()
    if wino:
        ra, ba = SB.wino_conv(gya, wa.flip(2, 3).transpose(0, 1), 1, wino)
        # the transposed product's output transform with the join's sum as its residual (BN-act form, no output maximum)
        assert len(Kn._seen.get("u2pl_gemm_batched_wsh_f32", ())) >= 2 and Kn._seen.get("u2pl_wino_output_bnact_f32")
    else:
        ra, ba = SB.conv_refs(x, wa, gya)["dx"]
        # the pointwise data gradient through the forward kernel's epilogue, the running sum as `res` (argument 23)
        assert any(c[23] is not None for c in Kn._seen.get("u2pl_conv2d_fwd_bnact_wsh_f32", ()))
    rb, bb = SB.conv_refs(x, wb, gyb)["dx"]
    _held("joined dx", xx.grad, ra + rb, ba + bb + SB.EPS * (ra.abs() + rb.abs()))


# ---- the maximum contract inside real steps ------------------------------------------------------------------------------------
# operand regions of the seven split-fp16 consumers (include/u2pl_hip.h): (tensor arg, ld arg, z-stride arg or None, amax arg,
# rows(args), cols(args), batch(args))
_REGIONS = {
    "u2pl_conv2d_fwd_wsh_f32": [(0, 1, None, 2, lambda a: a[7] * a[8] * a[9], lambda a: a[10], lambda a: 1)],
    "u2pl_conv2d_fwd_bnstats_wsh_f32": [(0, 1, None, 2, lambda a: a[7] * a[8] * a[9], lambda a: a[10], lambda a: 1)],
    "u2pl_conv2d_fwd_bnact_wsh_f32": [(0, 1, None, 2, lambda a: a[7] * a[8] * a[9], lambda a: a[10], lambda a: 1)],
    "u2pl_conv2d_dgrad_wsh_f32": [(0, 1, None, 2, lambda a: a[6] * a[10] * a[11], lambda a: a[12], lambda a: 1)],
    "u2pl_gemm_batched_wsh_f32": [(0, 1, 2, 3, lambda a: a[8], lambda a: a[9], lambda a: a[11])],
    "u2pl_conv2d_wgrad_h_f32": [(0, 1, None, 2, lambda a: a[9] * a[13] * a[14], lambda a: a[15], lambda a: 1),
                                (3, 4, None, 5, lambda a: a[9] * a[10] * a[11], lambda a: a[12], lambda a: 1)],
    "u2pl_wgrad_batched_h_f32": [(0, 1, 2, 3, lambda a: a[9], lambda a: a[11], lambda a: a[12]),
                                 (4, 5, 6, 7, lambda a: a[9], lambda a: a[10], lambda a: a[12])],
}


class AmaxChecker:
    """wraps u2pl_amd.nn.call: before each split-fp16 launch, synchronise (the weight gradients run on a side stream), read the
    operand region the kernel will read and the amax object's value, and record any maximum below the region's max |x| or, since
    every producer in nn.py is exact (stand-alone pass, BatchNorm apply / backward apply, Winograd transforms, eval epilogue),
    different from it.  Keeps range statistics of every operand; with `layers` (parameter -> name) it also recomputes the launches
    of those layers in float64 from the captured operands and holds their outputs to the element-wise bound (RealLaunchCheck)."""

    def __init__(self, real, layers=None):
        self.real = real
        self.count = {n: 0 for n in _REGIONS}
        self.below, self.inexact, self.stats = [], [], []
        self.verify = RealLaunchCheck(real, layers) if layers else None

    def __call__(self, name, *args):
        spec = _REGIONS.get(name)
        if spec is None or torch.cuda.is_current_stream_capturing():
            return self.real(name, *args)
        torch.cuda.synchronize()
        self.count[name] += 1
        ranges = []
        for which, (ti, li, zi, ai, rows, cols, batch) in enumerate(spec):
            region = _region(args, ti, li, zi, rows, cols, batch)
            true = region.abs().max()
            amax = args[ai].view(torch.int32).max().view(torch.float32)
            rec = (name, which, float(amax), float(true), tuple(region.shape))
            if bool(torch.isnan(true)):
                if not bool(torch.isnan(amax)):
                    self.below.append(rec)
            elif not bool(amax >= true):
                self.below.append(rec)
            elif not bool(amax == true):
                self.inexact.append(rec)
            ranges.append(_range_stats(name, which, region))
        self.stats.extend(ranges)
        job = self.verify.before(name, args) if self.verify is not None else None
        out = self.real(name, *args)
        if job is not None:
            torch.cuda.synchronize()
            self.verify.after(job, ranges)
        return out


def _region(args, ti, li, zi, rows, cols, batch):
    t, ld, z = args[ti], int(args[li]), int(args[zi]) if zi is not None else 0
    R, C, B = int(rows(args)), int(cols(args)), int(batch(args))
    return t.as_strided((B, R, C), (z, ld, 1), t.storage_offset())


def _nchw(t, ld, N, H, W, C):
    """rows [N*H*W][C] (pitch ld) at t's start -> float64 CPU [N][C][H][W]"""
    return t.as_strided((N, H, W, C), (H * W * ld, W * ld, ld, 1), t.storage_offset()).double().cpu().permute(0, 3, 1, 2)


class RealLaunchCheck:
    """float64 recomputation of captured real launches.  The layer is found from the launch's weight operand: the split planes
    (u2pl_amd.operands cache entries: kind fh / dh / wf{mt}h / wd{mt}h) or, for a weight gradient, the arena gradient view it
    writes.  One launch per (entry point, layer, Winograd setting) is recomputed.  u2pl_wgrad_batched_h_f32 writes slab partials
    of the Winograd-domain gradient: it is held to the bound by test_winograd_routes_meet_the_element_wise_bound, not here."""

    def __init__(self, real, layers):
        self.real, self.layers = real, layers       # layers: list of (name, parameter)
        self.done, self.records = set(), []

    def _by_plane(self, ptr):
        for n, p in self.layers:
            for kind, e in p.__dict__.get("_u2pl_derived", {}).items():
                if e["buf"].data_ptr() == ptr:
                    return n, p, kind
        return None

    def _by_sink(self, ptr):
        for n, p in self.layers:
            g = getattr(p, "_u2pl_grad", None)
            if g is not None and g.data_ptr() == ptr:
                return n, p, "sink"
        return None

    def before(self, name, a):
        from u2pl_amd import nn as Kn
        if name in ("u2pl_conv2d_fwd_wsh_f32", "u2pl_conv2d_fwd_bnstats_wsh_f32", "u2pl_conv2d_fwd_bnact_wsh_f32",
                    "u2pl_conv2d_dgrad_wsh_f32"):
            hit = self._by_plane(a[3].data_ptr())
        elif name == "u2pl_gemm_batched_wsh_f32":
            hit = self._by_plane(a[4].data_ptr())
        elif name == "u2pl_conv2d_wgrad_h_f32":
            hit = self._by_sink(a[6].data_ptr())
        else:
            hit = None
        if hit is None:
            return None
        key = (name, hit[0], Kn.CONV_ALGO["wino"], hit[2])
        if key in self.done:
            return None
        self.done.add(key)
        job = dict(name=name, layer=hit[0], p=hit[1], kind=hit[2], wino=Kn.CONV_ALGO["wino"], a=a)
        if name == "u2pl_conv2d_wgrad_h_f32":
            Cout, R, S, Cin = (int(a[i]) for i in (15, 16, 17, 12))
            job["prev"] = self._dw(a[6], Cout, R, S, Cin) if int(a[8]) else None
        return job

    @staticmethod
    def _dw(t, Cout, R, S, Cin):
        return t.as_strided((Cout, R, S, Cin), (R * S * Cin, S * Cin, Cin, 1), t.storage_offset()).double().cpu().permute(0, 3, 1, 2)

    def after(self, job, ranges):
        name, a, p = job["name"], job["a"], job["p"].detach()
        if name == "u2pl_gemm_batched_wsh_f32":
            got, ref, bound, K = self._batched(job)
        elif name == "u2pl_conv2d_dgrad_wsh_f32":
            N, Hin, Win, Cin, Ho, Wo, Cout, R, S, st, pd, dl = (int(a[i]) for i in range(6, 18))
            gy = _nchw(a[0], int(a[1]), N, Ho, Wo, Cout)
            ref, bound = SB.conv_dx_bound(gy, p, (Hin, Win), st, pd, dl)
            got, K = _nchw(a[4], int(a[5]), N, Hin, Win, Cin), R * S * Cout
        elif name == "u2pl_conv2d_wgrad_h_f32":
            N, Hin, Win, Cin, Ho, Wo, Cout, R, S, st, pd, dl = (int(a[i]) for i in range(9, 21))
            gy, x = _nchw(a[0], int(a[1]), N, Ho, Wo, Cout), _nchw(a[3], int(a[4]), N, Hin, Win, Cin)
            ref, bound = SB.conv_dw_bound(gy, x, (R, S), st, pd, dl)
            got, K = self._dw(a[6], Cout, R, S, Cin), N * Ho * Wo
            if job["prev"] is not None:         # accumulate = 1: sink = previous + dw, one more fp32 rounding
                bound = bound + SB.EPS * (job["prev"].abs() + ref.abs())
                ref = ref + job["prev"]
        else:
            N, Hin, Win, Cin, Ho, Wo, Cout, R, S, st, pd, dl = (int(a[i]) for i in range(7, 19))
            w = p if job["kind"].startswith("f") else p.transpose(0, 1)      # dh planes in the forward kernel: pointwise dgrad
            x = _nchw(a[0], int(a[1]), N, Hin, Win, Cin)
            ref, bound = SB.conv_y_bound(x, w, st, pd, dl)
            K = R * S * Cin
            if a[4] is not None:
                ref = ref + a[4].detach().double().cpu().view(1, -1, 1, 1)
                bound = bound + SB.EPS * ref.abs()
            if name == "u2pl_conv2d_fwd_bnact_wsh_f32":
                mean, invstd, gamma, beta = (a[i].detach().double().cpu().view(1, -1, 1, 1) for i in (19, 20, 21, 22))
                res = _nchw(a[23], int(a[24]), N, Ho, Wo, Cout) if a[23] is not None else torch.zeros_like(ref)
                sc = invstd * gamma
                bound = sc.abs() * bound + SB.C_EPI * SB.EPS * ((ref * sc).abs() + (mean * sc).abs() + beta.abs() + res.abs())
                ref = (ref - mean) * sc + beta + res
                if int(a[25]):
                    ref = torch.relu(ref)
            got = _nchw(a[5], int(a[6]), N, Ho, Wo, Cout)
        self.records.append(dict(entry=name, layer=job["layer"], wino=job["wino"], K=int(K), outputs=int(ref.numel()),
                                 excess=SB.excess(got, ref, bound), frac_self_rel_err_gt_2m16=SB.self_relative_fraction(got, ref),
                                 operands=[dict((k, r[k]) for k in ("shape", "max", "frac_below_2m17", "log10_span")) for r in ranges]))

    def _batched(self, job):
        a, p, kind = job["a"], job["p"], job["kind"]
        transposed, mt = kind.startswith("wd"), int(kind[2])
        Cout, Cin = p.shape[:2]
        a2 = (mt + 2) ** 2
        U = torch.empty(a2 * Cout * Cin, dtype=torch.float32, device=p.device)
        self.real("u2pl_wino_weight_f32", p.detach(), Cout, Cin, int(transposed), mt, U)     # the planes' fp32 source
        torch.cuda.synchronize()
        M, K, Nn, B = (int(a[i]) for i in (8, 9, 10, 11))
        U = U.double().cpu().view(a2, Nn, K)
        X = _region(a, 0, 1, 2, lambda _: M, lambda _: K, lambda _: B).double().cpu()
        got = a[5].as_strided((B, M, Nn), (int(a[7]), int(a[6]), 1), a[5].storage_offset()).double().cpu()
        Xa, Ua = X.abs(), U.abs()
        ref = X @ U.transpose(1, 2)
        bound = (SB.A_REL * SB.EPS * (Xa @ Ua.transpose(1, 2))
                 + SB.FLOOR * (float(Xa.max()) * (torch.ones_like(X) @ Ua.transpose(1, 2))
                               + Ua.amax(dim=(1, 2)).view(B, 1, 1) * (Xa @ torch.ones_like(U).transpose(1, 2))))
        return got, ref, bound, K


def _range_stats(name, which, region):
    a = region.detach().abs().double().flatten()
    nz = a[a > 0]
    m = float(a.max())
    return dict(entry=name, operand=which, shape=list(region.shape), max=m,
                frac_nonzero=float(nz.numel() / max(1, a.numel())),
                frac_below_2m17=float((nz < m * 2.0 ** -17).double().mean()) if nz.numel() else 0.0,
                log10_span=float(torch.log10(nz.max() / nz.min())) if nz.numel() else 0.0)


def _step_setup(S, seed, sup_only=True):
    from u2pl_amd import configs
    from u2pl_amd.models.model_helper import ModelBuilder
    from u2pl_amd.trainer import SemiTrainer
    from u2pl_amd.utils.loss_helper import get_criterion
    cfg = configs.cityscapes_semi(arch="resnet101", crop=S, batch_size=2, sync_bn=False, epochs=20)
    cfg["criterion"]["kwargs"]["min_kept"] = 2000
    cfg["trainer"]["contrastive"]["current_class_threshold"] = 0.055
    if sup_only:
        cfg["trainer"]["sup_only_epoch"] = 1
    torch.manual_seed(seed)
    model, teacher = ModelBuilder(cfg["net"]).to(DEV), ModelBuilder(cfg["net"]).to(DEV)
    tr = SemiTrainer(cfg, model, teacher, get_criterion(cfg), steps_per_epoch=1)
    return tr, model, teacher


def test_amax_contract_holds_at_every_split_fp16_launch_of_real_steps(monkeypatch):
    """R101, C = 19, 2 + 2 images at 129^2, eager (no graph capture): one supervised-only step, two semi-supervised steps (loss
    heads, OHEM, contrastive path), the same two with Winograd off, one evaluation forward (eval-BN epilogue).  At every launch of
    the seven split-fp16 consumers the maximum handed to the kernel equals the max |x| of the operand region it reads."""
    import bench
    from u2pl_amd import nn as Kn
    monkeypatch.setenv("U2PL_GRAPHS", "0")
    saved = (dict(Kn.CONV_ALGO), dict(Kn.CONV_WS), dict(Kn.CONV_H))
    Kn.CONV_H["on"] = True
    Kn.CONV_WS["on"] = True
    out_path = os.environ.get("U2PL_RANGE_STATS_OUT")        # optional: where to write the launch records
    S = 129
    tr, model, teacher = _step_setup(S, 3)
    # the launches recomputed in float64: heads (representation, aux, classifier), decoder 3x3s, ASPP, the last layer4 block
    layers = [(tag + n, q) for tag, m in (("", model), ("teacher.", teacher)) for n, q in m.named_parameters()
              if q.dim() == 4 and n.startswith(("decoder.", "auxor.", "encoder.layer4.2."))]
    chk = AmaxChecker(Kn.call, layers)
    monkeypatch.setattr(Kn, "call", chk)
    try:
        gen = torch.Generator(device=DEV).manual_seed(3)
        batches = [bench.synth_batch(2, S, 19, DEV, gen) for _ in range(3)]
        batches = bench.calibrate(model, teacher, batches, batches, 4.0)      # trained-like state (bench.py's workload)
        il, ll, iu = batches[0]
        tr.train_step(il, ll, iu, epoch=0)                             # supervised only
        for wino in (saved[0]["wino"] or 4, 0):
            Kn.CONV_ALGO.update(wino=wino)
            for il, ll, iu in batches[1:]:
                m = tr.train_step(il, ll, iu, epoch=1)
                torch.cuda.synchronize()
                assert torch.isfinite(m).all(), m
        Kn.CONV_ALGO.update(wino=saved[0]["wino"] or 4)
        model.eval()
        with torch.no_grad(), Kn.eval_invstd(model):
            out = model(batches[0][0], need_aux=False, need_rep=False)["pred"]
        torch.cuda.synchronize()
        assert torch.isfinite(out).all()
        model.train()
    finally:
        Kn.CONV_ALGO.update(saved[0])
        Kn.CONV_WS.update(saved[1])
        Kn.CONV_H.update(saved[2])
    recs = chk.verify.records
    print("split-fp16 launches checked per entry point:", chk.count)
    print("real launches recomputed in float64:", len(recs), "largest error / bound:", max(r["excess"] for r in recs))
    if out_path:
        _write_range_stats(out_path, chk)
    assert all(v > 0 for v in chk.count.values()), chk.count
    assert not chk.below, chk.below[:10]
    assert not chk.inexact, (len(chk.inexact), chk.inexact[:10])
    # the real operands against the element-wise bound: every recomputed launch, every entry point that has a float64 form here
    assert {r["entry"] for r in recs} == set(_REGIONS) - {"u2pl_wgrad_batched_h_f32"}, {r["entry"] for r in recs}
    assert {r["wino"] for r in recs if r["entry"] == "u2pl_gemm_batched_wsh_f32"} and any(r["wino"] == 0 for r in recs)
    bad = [(r["entry"], r["layer"], r["wino"], r["excess"]) for r in recs if not r["excess"] <= 1.0]
    assert not bad, bad


def _write_range_stats(path, chk):
    """every launch's operand ranges aggregated per entry point and operand, and the float64-recomputed launches one by one"""
    import json
    per = {}
    for r in chk.stats:
        k = f"{r['entry']}[{r['operand']}]"
        e = per.setdefault(k, dict(launches=0, max_frac_below_2m17=0.0, mean_frac_below_2m17=0.0, max_log10_span=0.0))
        e["launches"] += 1
        e["max_frac_below_2m17"] = max(e["max_frac_below_2m17"], r["frac_below_2m17"])
        e["mean_frac_below_2m17"] += r["frac_below_2m17"]
        e["max_log10_span"] = max(e["max_log10_span"], r["log10_span"])
    for e in per.values():
        e["mean_frac_below_2m17"] /= e["launches"]
    with open(path, "w") as f:
        json.dump(dict(commit=os.environ.get("U2PL_COMMIT", ""), counts=chk.count, per_operand=per,
                       recomputed_launches=chk.verify.records), f, indent=1)
