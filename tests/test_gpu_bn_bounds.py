"""-m gpu: every BatchNorm route of u2pl_amd/nn.py held ELEMENT-WISE to the float64 bound of tests/bn_bounds.py (INTEGRATION.md
section 4), reached through the module code the step uses (Kn.BatchNorm2d, Kn.conv_bn, Kn.eval_invstd), and the statistics of
every train-mode BatchNorm of real R101 steps at 769^2 held to the same bound.

BnProbe wraps u2pl_amd.nn.call.  It notes which producer wrote each buffer of partial sums, captures the pivot (the running_mean)
and the running statistics before each finalisation, and after every apply / backward launch recomputes the layer in float64 on
the device from the launch's own operands, recording each output's error over its bound.

Producers of the statistics: u2pl_bn_stats_f32 (stand-alone; M <= 64: the float64 two-pass kernel), the igemm_ws epilogue
(u2pl_conv2d_fwd_bnstats_wsh_f32 / _ws_f32), the conv.hip epilogue (u2pl_conv2d_fwd_bnstats_f32, Cout <= 64), the Winograd output
transform (u2pl_wino_output_f32 with partials).  Finishers: u2pl_bn_finish_finalize_f32, and u2pl_colreduce_finish_f32 +
u2pl_bn_finalize_f32 (the SyncBatchNorm arithmetic)."""
import itertools
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn_bounds as BB  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
CL = torch.channels_last
VARIANTS = {"plain": (False, False, False), "res": (True, False, False), "relu": (False, True, False),
            "relu+drop": (False, True, True), "res+relu": (True, True, False)}      # (res, relu, drop)
# statistics producers: entry point -> (route, bias argument, partials argument, L(args)).  The Winograd transform's terms are
# fl(y - p) of the stored y: no bias shift.
_PRODUCERS = {
    "u2pl_conv2d_fwd_bnstats_wsh_f32": ("igemm_ws", 4, 20, lambda a: BB.L_IGEMM_WS),
    "u2pl_conv2d_fwd_bnstats_ws_f32": ("igemm_ws", 3, 19, lambda a: BB.L_IGEMM_WS),
    "u2pl_conv2d_fwd_bnstats_f32": ("conv", 3, 19, lambda a: BB.L_CONV),
    "u2pl_wino_output_f32": ("wino", None, 10, lambda a: BB.L_wino(int(a[6]), int(a[4]))),
}
_BWD = ("u2pl_bn_bwd_sums_f32", "u2pl_bn_bwd_sums_mx_f32", "u2pl_bn_bwd_apply_f32", "u2pl_bn_bwd_apply_pg_f32",
        "u2pl_bn_bwd_apply_amax_f32", "u2pl_sums_to_f32")


def _rows(t, ld, M, C):
    """rows [M][C] (pitch ld) at t's start, float64 on the device"""
    return t.as_strided((int(M), int(C)), (int(ld), 1), t.storage_offset()).double()


def _excess(got, ref, bound):
    """split_bounds.excess on the device"""
    got = got.detach().double().reshape(ref.shape)
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    return float(((got - ref).abs() / (bound + 1e-300)).max())


class BnProbe:
    """wraps u2pl_amd.nn.call (see the module docstring).  records: one dict per checked launch (entry, route, finisher, M, C,
    R statistics, excess per output); unknown: launches it could not attribute -- eval-mode applies whose invstd came from the
    one-launch eval_invstd form (train False), train-mode applies whose statistics had no known producer and statistics
    producers it has no summation order for (train True)."""

    def __init__(self, real, backward=True, names=None):
        self.real, self.backward, self.names = real, backward, names or {}
        self.seen, self.src, self.fwd, self.evals, self.info, self.bsums = {}, {}, {}, {}, {}, {}
        self.records, self.unknown = [], []

    def __call__(self, name, *a):
        self.seen[name] = self.seen.get(name, 0) + 1
        if "bnstats" in name and name not in _PRODUCERS:     # a statistics producer whose summation order has no L here
            self.unknown.append(dict(entry=name, mode="producer", train=True))
        h = _HANDLERS.get(name)
        if h is None or torch.cuda.is_current_stream_capturing() or (not self.backward and name in _BWD):
            return self.real(name, *a)
        return h(self, name, a)

    # ---- forward -------------------------------------------------------------------------------------------------------------
    def _producer(self, name, a):
        route, bi, pi, L = _PRODUCERS[name]
        if a[pi] is not None:
            bias = a[bi] if bi is not None else None
            self.src[a[pi].data_ptr()] = (route, L(a), None if bias is None else bias.detach().double().clone())
        return self.real(name, *a)

    def _finish(self, name, a):
        self.src[a[3].data_ptr()] = self.src.pop(a[0].data_ptr(), None)
        return self.real(name, *a)

    def _stats(self, name, a):
        M, C = int(a[2]), int(a[3])
        self.src[a[6].data_ptr()] = ("small", None, None) if M <= BB.SMALL_M else ("standalone", BB.L_standalone(M, C), None)
        return self.real(name, *a)

    def _finalize(self, name, a):
        if name == "u2pl_bn_finalize_f32":
            src, count, pivot, eps, mom, invstd, rm, rv = a[0], a[1], a[2], a[4], a[5], a[7], a[8], a[9]
        else:
            src, count, pivot, eps, mom, invstd, rm, rv = a[0], a[3], a[4], a[5], a[6], a[8], a[9], a[10]
        torch.cuda.synchronize()
        before = (pivot.detach().double().clone(), rm.detach().double().clone(), rv.detach().double().clone())
        out = self.real(name, *a)
        torch.cuda.synchronize()
        # (each entry is consumed here: a buffer the allocator hands out again at the same address never inherits a route)
        self.fwd[invstd.data_ptr()] = dict(finisher=name, src=self.src.pop(src.data_ptr(), None), p=before[0], rm0=before[1],
                                           rv0=before[2], rm=rm.detach().double().clone(), rv=rv.detach().double().clone(),
                                           eps=float(np.float32(eps)), mom=float(mom), count=float(count),
                                           layer=self.names.get(pivot.data_ptr(), "?"))
        return out

    def _eval_prep(self, name, a):
        out = self.real(name, *a)
        torch.cuda.synchronize()
        self.evals[a[3].data_ptr()] = (a[0].detach().double().clone(), float(np.float32(a[2])))
        return out

    def _apply(self, name, a):
        x, ldx, mean, invstd, gamma, beta, res, ldr, relu, drop, hw, y, ldy, M, C = a[:15]
        out = self.real(name, *a)
        torch.cuda.synchronize()
        M, C, hw, relu = int(M), int(C), int(hw), bool(relu)
        f = self.fwd.pop(invstd.data_ptr(), None)
        ev = self.evals.pop(invstd.data_ptr(), None)
        rec = dict(entry=name, M=M, C=C, relu=relu, res=res is not None, drop=drop is not None, train=f is not None)
        if (f is None or f["src"] is None) and ev is None:
            self.unknown.append(rec)
            return out
        X = _rows(x, ldx, M, C)
        if f is not None:
            route, L, bias = f["src"]
            P = f["p"]
            shift = BB.bias_shift_err(X, bias, P) if bias is not None else None
            mu, var = BB.stats_ref(X)
            e_mu, e_var, e1 = BB.stats_bound(X, P, L, shift)
            iota, e_iota, hi = BB.invstd_interval(var, e_var, f["eps"])
            rm, brm, rv, brv = BB.running_ref_bound(f["rm0"], f["rv0"], mu, var, f["count"], f["mom"], e1, e_var)
            sd = var.sqrt()
            live = sd > 0
            Rc = ((mu - P).abs() / sd)[live]
            # the fp32-only part of the bound: the same route with the pivot at the mean (R = 0)
            _, e_var0, _ = BB.stats_bound(X, mu, L, shift)
            _, e_iota0, _ = BB.invstd_interval(var, e_var0, f["eps"])
            got_iota = invstd.detach().double()
            rec.update(mode="train", route=route, L=L, finisher=f["finisher"], layer=f["layer"], bias=bias is not None,
                       R_max=float(Rc.max()) if Rc.numel() else 0.0,
                       R_p99=float(torch.quantile(Rc, 0.99)) if Rc.numel() else 0.0, const_channels=int((~live).sum()),
                       invstd_err_over_fp32_part=float(((got_iota - iota).abs() / e_iota0).max()),
                       kernel_invstd=got_iota.clone(),
                       excess=dict(mean=_excess(mean, mu, e_mu), invstd=_excess(invstd, iota, e_iota),
                                   running_mean=_excess(f["rm"], rm, brm), running_var=_excess(f["rv"], rv, brv)))
        else:
            rv0, eps = ev
            iota = 1.0 / torch.sqrt(rv0 + eps)
            e_iota = (BB.EPS + 4 * BB.D64) * iota
            hi = iota + e_iota
            mu, e_mu = mean.detach().double(), torch.zeros_like(iota)
            ulp = (torch.nextafter(invstd.detach(), torch.full_like(invstd, float("inf"))) - invstd.detach()).double()
            rec.update(mode="eval", excess=dict(invstd=_excess(invstd, iota, e_iota),
                                                invstd_1ulp=float(((invstd.double() - iota).abs() / ulp).max())))
        G, B = gamma.detach().double(), beta.detach().double()
        RES = _rows(res, ldr, M, C) if res is not None else None
        DR = drop.detach().double().repeat_interleave(hw, 0) if drop is not None else None
        Y = _rows(y, ldy, M, C)
        pre, b = BB.apply_ref_bound(X, mu, iota, e_mu, e_iota, hi, G, B, RES)
        yr, by = BB.finish_y(pre, b, relu, DR)
        rec["excess"]["y"] = _excess(Y, yr, by)
        rec["mask_mismatch"] = BB.mask_mismatch(pre, b, Y, DR) if relu else 0
        self.records.append(rec)
        if self.backward:
            self.info[invstd.data_ptr()] = dict(mu=mu, e_mu=e_mu, iota=iota, e_iota=e_iota, hi=hi, mode=rec["mode"],
                                                mask=(Y > 0) if relu else None)
        return out

    # ---- backward ------------------------------------------------------------------------------------------------------------
    def _bw(self, f, gy, ldg, x, ldx, drop, hw, M, C, gamma, masked):
        M, C, hw = int(M), int(C), int(hw)
        X, DY = _rows(x, ldx, M, C), _rows(gy, ldg, M, C)
        DR = drop.detach().double().repeat_interleave(hw, 0) if drop is not None else None
        assert not masked or f["mask"] is not None, "a masked backward of a forward without ReLU"
        mask = f["mask"].double() if masked else 1.0      # the kernel's own forward decision
        G = gamma.detach().double() if gamma is not None else torch.ones(C, dtype=torch.float64, device=X.device)
        bw = BB.bwd_ref_bound(X, DY, mask, DR, f["mu"], f["iota"], f["e_mu"], f["e_iota"], f["hi"], G, BB.L_colreduce_chain(M, C))
        if f["mode"] == "eval":
            bw["dx"] = BB.eval_bwd_ref_bound(DY, mask, DR, f["iota"], f["e_iota"], f["hi"], G)
        return bw

    def _bwd_sums(self, name, a):
        out = self.real(name, *a)
        torch.cuda.synchronize()
        if name == "u2pl_bn_bwd_sums_f32":
            invstd, drop, hw, M, C, sums, masked = a[7], a[8], a[9], a[10], a[11], a[13], a[4] is not None
        else:
            invstd, drop, hw, M, C, sums, masked = a[5], a[8], a[9], a[10], a[11], a[13], True
        rec = dict(entry=name, mode="bwd_sums", M=int(M), C=int(C))
        f = self.info.get(invstd.data_ptr())
        if f is None:
            self.unknown.append(rec)
            return out
        C = int(C)
        bw = self._bw(f, a[0], a[1], a[2], a[3], drop, hw, M, C, None, masked)
        S = sums.detach().double()
        rec["excess"] = dict(S0=_excess(S[:C], *bw["S0"]), S1=_excess(S[C:2 * C], *bw["S1"]))
        self.records.append(rec)
        self.bsums = {sums.data_ptr(): (C, bw["S0"], bw["S1"])}      # this layer's; the sums_to calls that follow read it
        return out

    def _sums_to(self, name, a):
        s, acc, dst = a[0], int(a[3]), a[4]
        old = dst.detach().double().clone() if acc else None
        out = self.real(name, *a)
        hit = None
        for base, (C, S0, S1) in self.bsums.items():
            if s.data_ptr() == base:
                hit = ("dbeta", S0)
            elif s.data_ptr() == base + 8 * C:
                hit = ("dgamma", S1)
        if hit is None:
            return out
        torch.cuda.synchronize()
        ref, e = hit[1]
        bound = e * (1 + BB.EPS) + BB.EPS * ref.abs()
        if old is not None:          # accumulate = 1: one more rounding of the sum
            bound, ref = bound + BB.EPS * (ref.abs() + old.abs()), ref + old
        self.records.append(dict(entry=name, mode="param", accumulate=acc, excess={hit[0]: _excess(dst, ref, bound)}))
        return out

    def _bwd_apply(self, name, a):
        gy, ldg, x, ldx, y, ldy, mean, invstd, gamma, drop, hw, sums, count, dx, lddx, dres, lddr, M, C = a[:19]
        psums = a[19] if len(a) > 19 else None
        gsink, bsink, acc = (a[20], a[21], int(a[22])) if len(a) > 22 else (None, None, 0)
        relu_beta = a[25] if len(a) > 25 else None
        old = (gsink.detach().double().clone(), bsink.detach().double().clone()) if psums is not None and acc else None
        out = self.real(name, *a)
        torch.cuda.synchronize()
        self.bsums = {}
        M, C = int(M), int(C)
        rec = dict(entry=name, mode="bwd", M=M, C=C, mask="x" if relu_beta is not None else ("y" if y is not None else None),
                   pg=psums is not None, train=sums is not None)
        f = self.info.get(invstd.data_ptr())
        if f is None:
            self.unknown.append(rec)
            return out
        bw = self._bw(f, gy, ldg, x, ldx, drop, hw, M, C, gamma, y is not None or relu_beta is not None)
        ex = dict(dx=_excess(_rows(dx, lddx, M, C), *bw["dx"]))
        if sums is not None:
            S = sums.detach().double()
            ex.update(S0=_excess(S[:C], *bw["S0"]), S1=_excess(S[C:2 * C], *bw["S1"]))
        if dres is not None:
            ex["dres"] = _excess(_rows(dres, lddr, M, C), *bw["dres"])
        if psums is not None:       # dgamma = S1, dbeta = S0 written into the arena sinks by the same launch
            for key, sink, (ref, e), prev in (("dgamma_sink", gsink, bw["S1"], old[0] if old else None),
                                              ("dbeta_sink", bsink, bw["S0"], old[1] if old else None)):
                bound = e * (1 + BB.EPS) + BB.EPS * ref.abs()
                if prev is not None:
                    bound, ref = bound + BB.EPS * (ref.abs() + prev.abs()), ref + prev
                ex[key] = _excess(sink, ref, bound)
        rec["excess"] = ex
        self.records.append(rec)
        return out


_HANDLERS = {n: BnProbe._producer for n in _PRODUCERS}
_HANDLERS.update({"u2pl_colreduce_finish_f32": BnProbe._finish, "u2pl_bn_stats_f32": BnProbe._stats,
                  "u2pl_bn_finalize_f32": BnProbe._finalize, "u2pl_bn_finish_finalize_f32": BnProbe._finalize,
                  "u2pl_bn_eval_invstd_f32": BnProbe._eval_prep, "u2pl_bn_apply_f32": BnProbe._apply,
                  "u2pl_bn_apply_amax_f32": BnProbe._apply, "u2pl_bn_bwd_sums_f32": BnProbe._bwd_sums,
                  "u2pl_bn_bwd_sums_mx_f32": BnProbe._bwd_sums, "u2pl_sums_to_f32": BnProbe._sums_to,
                  "u2pl_bn_bwd_apply_f32": BnProbe._bwd_apply, "u2pl_bn_bwd_apply_pg_f32": BnProbe._bwd_apply,
                  "u2pl_bn_bwd_apply_amax_f32": BnProbe._bwd_apply})


def _bad(probe):
    return [(r["entry"], r.get("route"), r.get("layer"), k, v) for r in probe.records for k, v in r["excess"].items()
            if not v <= 1.0 and k != "invstd_1ulp"]


def _held(probe):
    bad = _bad(probe)
    assert not bad, bad[:10]
    mm = [(r["entry"], r.get("route"), r["mask_mismatch"]) for r in probe.records if r.get("mask_mismatch")]
    assert not mm, mm[:10]
    assert not probe.unknown, probe.unknown[:5]


@pytest.fixture
def Kn(monkeypatch):
    """a BnProbe around u2pl_amd.nn.call; every switch a test turns restored afterwards"""
    from u2pl_amd import nn as K
    saved = (dict(K.CONV_ALGO), dict(K.CONV_WS), dict(K.CONV_H), K.FUSE_BN_FINISH, K.RELU_MASK_FROM_X)
    probe = BnProbe(K.call)
    monkeypatch.setattr(K, "call", probe)
    monkeypatch.setattr(K, "_probe", probe, raising=False)
    yield K
    K.CONV_ALGO.update(saved[0])
    K.CONV_WS.update(saved[1])
    K.CONV_H.update(saved[2])
    K.FUSE_BN_FINISH, K.RELU_MASK_FROM_X = saved[3], saved[4]


def _bn(Kn, C, g):
    bn = Kn.BatchNorm2d(C).to(DEV)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(C, generator=g, device=DEV) + 0.5)
        bn.bias.copy_(torch.randn(C, generator=g, device=DEV) * 0.1)
        bn.running_var.copy_(torch.rand(C, generator=g, device=DEV) + 0.5)
    return bn


def _x(N, C, H, g):
    mu = torch.randn(C, generator=g, device=DEV) * 2
    sd = torch.rand(C, generator=g, device=DEV) + 0.5
    x = torch.randn(N, C, H, H, generator=g, device=DEV) * sd.view(1, C, 1, 1) + mu.view(1, C, 1, 1)
    return x.contiguous(memory_format=CL)


def _set_pivot(bn, y, R, g, const=None):
    """running_mean = mu + R sigma per channel of y (random sign); `const`: channels whose pivot is moved off their value"""
    yd = y.detach().double()
    mu, sd = yd.mean((0, 2, 3)), yd.std((0, 2, 3), unbiased=False)
    sign = torch.where(torch.rand(mu.shape, generator=g, device=DEV) < 0.5, -1.0, 1.0).double()
    p = mu + R * sd * sign
    if const is not None:
        p[const] = mu[const] + 0.75
    with torch.no_grad():
        bn.running_mean.copy_(p.float())


def _step(out, g):
    """backward of one call with a random output gradient"""
    out.backward(torch.randn(out.shape, generator=g, device=DEV).contiguous(memory_format=CL))
    torch.cuda.synchronize()


def _inputs(variant, N, C, H, g):
    res, relu, drop = VARIANTS[variant]
    rr = torch.randn(N, C, H, H, generator=g, device=DEV).contiguous(memory_format=CL).requires_grad_(True) if res else None
    dm = ((torch.rand(N, C, generator=g, device=DEV) > 0.3).float() / 0.7) if drop else None
    return rr, relu, dm


def _switch(Kn, k):
    """call k of 10: split-fp16 on for the first five (the _amax forms, the backward's mask from x where there is no residual),
    off for the last five (the plain forms, the mask from y); the fused finish on every other call"""
    form = k < 5
    Kn.CONV_H["on"] = form
    Kn.RELU_MASK_FROM_X = form
    Kn.FUSE_BN_FINISH = k % 2 == 0


# ---- stand-alone statistics (M > 64) --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,H,N", [(64, 385, 4), (128, 385, 4), (36, 31, 3), (320, 29, 2)])
def test_standalone_statistics_route(C, H, N, Kn):
    """u2pl_bn_stats_f32 at the stem's size (385^2 x 4 rows), C/4 not a power of two, a ragged second column slab; every apply
    variant in both forms, the backward with the mask from y and from x, the parameter gradients into plain tensors (first
    half) and into arena sinks (second half, fused into the apply launch or by u2pl_sums_to_f32 with accumulate = 1)"""
    g = torch.Generator(device=DEV).manual_seed(C + H + N)
    bn = _bn(Kn, C, g)
    for k, variant in enumerate(itertools.chain(VARIANTS, VARIANTS)):
        _switch(Kn, k)
        if k == 5:
            Kn.ParamArena([[bn.weight, bn.bias]])
        x = _x(N, C, H, g).requires_grad_(True)
        _set_pivot(bn, x, 1.0, g)
        rr, relu, dm = _inputs(variant, N, C, H, g)
        _step(bn(x, res=rr, relu=relu, drop=dm), g)
    p = Kn._probe
    _held(p)
    train = [r for r in p.records if r.get("mode") == "train"]
    assert len(train) == 10 and {r["route"] for r in train} == {"standalone"}
    assert {r["entry"] for r in train} == {"u2pl_bn_apply_amax_f32", "u2pl_bn_apply_f32"}
    assert {r["mask"] for r in p.records if r.get("mode") == "bwd"} == {"x", "y", None}
    assert {r["entry"] for r in p.records if r.get("mode") == "bwd"} == {"u2pl_bn_bwd_apply_amax_f32", "u2pl_bn_bwd_apply_pg_f32",
                                                                          "u2pl_bn_bwd_apply_f32"}
    assert {r["accumulate"] for r in p.records if r.get("mode") == "param"} == {0, 1}


# ---- few rows: the pooled ASPP branch -------------------------------------------------------------------------------------------
def _pooled(N, C, g):
    base = torch.rand(C, generator=g, device=DEV) + 0.5
    return (base * (1 + 0.01 * torch.randn(N, C, generator=g, device=DEV))).view(N, C, 1, 1).contiguous(memory_format=CL)


@pytest.mark.parametrize("N", [2, 4, 16])
def test_few_row_statistics_route(N, Kn):
    """(256, 1, N): pooled vectors whose rows differ by ~1 % with the pivot at 0 (R ~ 100): k_bn_stats_small, held to its
    double-precision bound, forward and backward, both forms"""
    g = torch.Generator(device=DEV).manual_seed(N)
    bn = _bn(Kn, 256, g)
    for k in range(2):
        _switch(Kn, 5 * k)
        with torch.no_grad():
            bn.running_mean.zero_()
        x = _pooled(N, 256, g).requires_grad_(True)
        _step(bn(x, relu=True), g)
    p = Kn._probe
    _held(p)
    train = [r for r in p.records if r.get("mode") == "train"]
    assert {r["route"] for r in train} == {"small"} and min(r["R_max"] for r in train) > 30


def test_few_row_switch_sits_between_64_and_65_rows(Kn):
    """the same rows at M = 64 (float64 two-pass kernel) and M = 65 (fp32 column reduction): each meets its own route's bound,
    and at M = 65 the kernel's invstd misses the double-precision bound (the fp32 route did run)"""
    g = torch.Generator(device=DEV).manual_seed(64)
    rows = _pooled(65, 256, g)
    routes = {}
    for M in (64, 65):
        bn = _bn(Kn, 256, g)
        with torch.no_grad():
            bn.running_mean.zero_()
        x = rows[:M].contiguous(memory_format=CL)
        with torch.no_grad():
            bn(x, relu=True)
        torch.cuda.synchronize()
        rec = Kn._probe.records[-1]
        routes[M] = rec["route"]
        X = x.detach().double().reshape(M, 256)
        _, var = BB.stats_ref(X)
        _, e_small, _ = BB.stats_bound(X, torch.zeros(256, dtype=torch.float64, device=DEV), None)
        iota, e_iota, _ = BB.invstd_interval(var, e_small, float(np.float32(bn.eps)))
        routes[f"double_bound_{M}"] = _excess(rec["kernel_invstd"], iota, e_iota)
    _held(Kn._probe)
    assert routes[64] == "small" and routes[65] == "standalone", routes
    assert routes["double_bound_64"] <= 1.0 and routes["double_bound_65"] > 1.0, routes


# ---- fused statistics: the conv epilogues and the Winograd output transform -----------------------------------------------------
PRODUCERS = [  # (name, Cin, Cout, k, dil, H, N, bias, wino, route)
    ("ws 1x1 1024-256", 1024, 256, 1, 1, 97, 4, False, 0, "igemm_ws"),
    ("ws 1x1 256-1024", 256, 1024, 1, 1, 97, 4, False, 0, "igemm_ws"),
    ("ws 1x1 256-256 bias (decoder low_conv)", 256, 256, 1, 1, 193, 4, True, 0, "igemm_ws"),
    ("conv.hip 1x1 256-64 (layer1 conv1)", 256, 64, 1, 1, 193, 4, False, 0, "conv"),
    ("conv.hip 3x3 64-64 (layer1 conv2)", 64, 64, 3, 1, 193, 4, False, 0, "conv"),
    ("wino 3x3 d2 256-256", 256, 256, 3, 2, 97, 4, False, 4, "wino"),
    ("wino 3x3 512-256 bias (decoder head)", 512, 256, 3, 1, 193, 4, True, 4, "wino"),
]


@pytest.mark.parametrize("name,Cin,Cout,k,dil,H,N,bias,wino,route", PRODUCERS, ids=[p[0] for p in PRODUCERS])
def test_fused_statistics_producers(name, Cin, Cout, k, dil, H, N, bias, wino, route, Kn):
    """Kn.conv_bn with the statistics from the producer's epilogue (M = 4 x 97^2 = 37636 and 4 x 193^2 rows: not multiples of
    128), both finishers, every apply variant in both forms, the backward's sums / apply forms into arena sinks"""
    Kn.CONV_ALGO.update(wino=wino)
    g = torch.Generator(device=DEV).manual_seed(Cin + Cout + k + H)
    conv = Kn.Conv2d(Cin, Cout, k, padding=dil * (k // 2), dilation=dil, bias=bias).to(DEV)
    bn = _bn(Kn, Cout, g)
    Kn.ParamArena([[conv.weight] + ([conv.bias] if bias else []), [bn.weight, bn.bias]])
    x = torch.relu(torch.randn(N, Cin, H, H, generator=g, device=DEV)).contiguous(memory_format=CL)   # post-ReLU: means != 0
    for kk, variant in enumerate(itertools.chain(VARIANTS, VARIANTS)):
        _switch(Kn, kk)
        rr, relu, dm = _inputs(variant, N, Cout, H, g)
        _step(Kn.conv_bn(conv, bn, x, res=rr, relu=relu, drop=dm), g)
        Kn.wgrad_stream_sync()
    torch.cuda.synchronize()
    p = Kn._probe
    _held(p)
    train = [r for r in p.records if r.get("mode") == "train"]
    assert len(train) == 10 and {r["route"] for r in train} == {route}, {r["route"] for r in train}
    assert {r["finisher"] for r in train} == {"u2pl_bn_finish_finalize_f32", "u2pl_bn_finalize_f32"}
    assert p.seen.get("u2pl_colreduce_finish_f32") and (bias or not any(r["bias"] for r in train))
    assert {r["entry"] for r in train} == {"u2pl_bn_apply_amax_f32", "u2pl_bn_apply_f32"}
    # every entry point of the table ran: the producer in both forms where it has two, both backward-sum forms (mask from x:
    # ReLU without a residual under the first five calls' switch), the three backward-apply forms
    names = {"igemm_ws": ("u2pl_conv2d_fwd_bnstats_wsh_f32", "u2pl_conv2d_fwd_bnstats_ws_f32"),
             "conv": ("u2pl_conv2d_fwd_bnstats_f32",), "wino": ("u2pl_wino_output_f32",)}[route]
    names += ("u2pl_bn_finish_finalize_f32", "u2pl_colreduce_finish_f32", "u2pl_bn_finalize_f32", "u2pl_bn_bwd_sums_f32",
              "u2pl_bn_bwd_sums_mx_f32", "u2pl_bn_bwd_apply_amax_f32", "u2pl_bn_bwd_apply_pg_f32", "u2pl_bn_bwd_apply_f32",
              "u2pl_sums_to_f32")
    assert all(p.seen.get(n) for n in names), {n: p.seen.get(n) for n in names}
    print(name, "largest error / bound:", max(v for r in p.records for v in r["excess"].values()),
          "R max:", max(r["R_max"] for r in train))


# ---- R sweep at a layer1-sized shape ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["standalone", "igemm_ws", "wino"])
def test_pivot_distance_sweep(route, Kn):
    """C = 64 / 256 at 193^2 x 4 rows: running_mean = mu + R sigma before the call, R in {0, 1, 10, 100, 1000}, with constant
    channels (pivot off their value).  The bound holds at every R; printed: the measured invstd error over the bound's fp32-only
    part (the same route at R = 0)"""
    g = torch.Generator(device=DEV).manual_seed(7)
    N, H = 4, 193
    Kn.CONV_ALGO.update(wino=4 if route == "wino" else 0)
    if route == "standalone":
        C = 64
        x = _x(N, C, H, g)
        x[:, :2] = 1.7
        conv = None
    else:
        Cin, C, k = (64, 256, 1) if route == "igemm_ws" else (64, 64, 3)
        conv = Kn.Conv2d(Cin, C, k, padding=k // 2, bias=route == "igemm_ws").to(DEV)
        with torch.no_grad():
            conv.weight[:2].zero_()          # channels 0, 1: constant (the bias, or 0)
        x = torch.relu(torch.randn(N, Cin, H, H, generator=g, device=DEV)).contiguous(memory_format=CL)
    bn = _bn(Kn, C, g)
    out = {}
    for R in (0, 1, 10, 100, 1000):
        with torch.no_grad():
            y = conv(x) if conv is not None else x
            _set_pivot(bn, y, R, g, const=[0, 1])
            Kn._probe.records.clear()
            bn.train()
            yy = Kn.conv_bn(conv, bn, x, relu=True) if conv is not None else bn(x, relu=True)
        torch.cuda.synchronize()
        del yy
        rec = [r for r in Kn._probe.records if r.get("mode") == "train"][-1]
        assert rec["route"] == route and rec["const_channels"] >= 2, rec
        out[R] = (rec["R_max"], max(rec["excess"].values()), rec["invstd_err_over_fp32_part"])
        _held(Kn._probe)
    print(route, "R -> (measured R max, largest error / bound, invstd error / fp32-only part):", out)
    assert out[1000][0] > 500


# ---- eval mode ------------------------------------------------------------------------------------------------------------------
def test_eval_mode_routes(Kn):
    """eval-mode BatchNorm with a recorded graph: invstd = u2pl_bn_eval_invstd_f32 (within 1 ulp of float64), apply with
    running_mean, backward dx = gamma invstd g; plain / res / relu / res + relu in both forms"""
    g = torch.Generator(device=DEV).manual_seed(11)
    N, C, H = 2, 256, 29
    bn = _bn(Kn, C, g)
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(C, generator=g, device=DEV))
        bn.running_var.copy_(10.0 ** (torch.rand(C, generator=g, device=DEV) * 8 - 5))     # 1e-5 .. 1e3
    bn.eval()
    for k, variant in enumerate(("plain", "res", "relu", "res+relu") * 2):
        _switch(Kn, 0 if k < 4 else 5)
        if k == 4:
            Kn.ParamArena([[bn.weight, bn.bias]])
        x = _x(N, C, H, g).requires_grad_(True)
        rr, relu, dm = _inputs(variant, N, C, H, g)
        _step(bn(x, res=rr, relu=relu), g)
    p = Kn._probe
    _held(p)
    ev = [r for r in p.records if r.get("mode") == "eval"]
    assert len(ev) == 8 and max(r["excess"]["invstd_1ulp"] for r in ev) <= 1.0
    assert not any(r["train"] for r in p.records if r.get("mode") == "bwd")


def test_eval_invstd_of_a_whole_model_in_one_launch(Kn):
    """u2pl_bn_eval_invstd_multi_f32 (Kn.eval_invstd): every BatchNorm's invstd within 1 ulp of float64, running_var over ten
    decades and a non-default eps"""
    g = torch.Generator(device=DEV).manual_seed(12)
    bns = [_bn(Kn, C, g) for C in (64, 36, 2048, 256)]
    bns[1].eps = 1e-3
    with torch.no_grad():
        for b in bns:
            b.running_var.copy_(10.0 ** (torch.rand(b.num_features, generator=g, device=DEV) * 10 - 6))
    model = torch.nn.Sequential(*bns).eval()
    with Kn.eval_invstd(model):
        views = [Kn._EVAL_INVSTD[id(b)].clone() for b in bns]
    torch.cuda.synchronize()
    assert Kn._probe.seen.get("u2pl_bn_eval_invstd_multi_f32")
    for b, v in zip(bns, views):
        ref = 1.0 / torch.sqrt(b.running_var.double() + float(np.float32(b.eps)))
        ulp = (torch.nextafter(v, torch.full_like(v, float("inf"))) - v).double()
        assert float(((v.double() - ref).abs() / ulp).max()) <= 1.0


# ---- the pooled branch end to end -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [2, 4, 16])
def test_pooled_branch_end_to_end(N, Kn):
    """GAP -> 1x1 2048 -> 256 (u2pl_dense_small_f32, float64 accumulation) -> BatchNorm over M = N rows (k_bn_stats_small) ->
    ReLU -> broadcast.  Forward: the GAP within its fp32 column-reduction bound, the dense output within 1 ulp of the float64 dot
    product of its operands, the broadcast exact, and the branch output within the float64 chain's bound carried from x.
    Backward: the BatchNorm's sums, dx and parameter gradients held by the probe."""
    g = torch.Generator(device=DEV).manual_seed(100 + N)
    H = 13
    x = torch.relu(torch.randn(N, 2048, H, H, generator=g, device=DEV)).contiguous(memory_format=CL).requires_grad_(True)
    conv = Kn.Conv2d(2048, 256, 1, bias=False).to(DEV)
    bn = _bn(Kn, 256, g)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g, device=DEV) / 2048 ** 0.5)
        bn.running_mean.zero_()
    pooled = Kn.global_avg_pool(x)
    z = Kn.conv_bn(conv, bn, pooled, relu=True)
    up = Kn.upsample_bilinear(z, (H, H))
    xb = z.grad_fn.saved_tensors[0].detach().double().reshape(N, 256)     # the BatchNorm's input: the dense layer's output
    _step(up, g)
    p = Kn._probe
    assert p.seen.get("u2pl_dense_small_f32") and p.seen.get("u2pl_bn_stats_f32")
    _held(p)
    train = [r for r in p.records if r.get("mode") == "train"]
    assert [r["route"] for r in train] == ["small"] and train[0]["R_max"] > 10      # pooled rows: the pivot (0) far off
    assert {r["mode"] for r in p.records} >= {"bwd_sums", "bwd"}
    assert torch.equal(up.detach()[:, :, 3, 5], z.detach()[:, :, 0, 0])
    # GAP: SumOp terms through the column-reduction chain, then the fp32 scale 1/(H W) and the cast (2 roundings)
    X64 = x.detach().double()
    gap = X64.mean((2, 3))
    e_gap = BB.L_colreduce_chain(H * H, 2048) * BB.EPS * X64.abs().mean((2, 3)) + 2 * BB.EPS * gap.abs()
    P = pooled.detach().double().reshape(N, 2048)
    assert _excess(P, gap, e_gap) <= 1.0
    # the dense layer on the kernel's own pooled vector: within 1 ulp
    W = conv.weight.detach().double().reshape(256, 2048)
    dense = P @ W.T
    ulp = (torch.nextafter(xb.float(), torch.full_like(xb.float(), float("inf"))) - xb.float()).double()
    assert float(((xb - dense).abs() / ulp).max()) <= 1.0
    # the branch output against float64 from x: the input error e_d = |W| e_gap + 1 ulp carried through the normalisation to
    # first order (d xhat_i = iota (e_i - mean e - xhat_i mean(xhat e)); e_d is ~1e-5 of sigma here, the second order ~1e-10),
    # plus the BatchNorm's own bound on its kernel input
    d64 = gap @ W.T
    e_d = e_gap @ W.abs().T + ulp
    mu, var = BB.stats_ref(d64)
    iota = 1.0 / torch.sqrt(var + float(np.float32(bn.eps)))
    xh = (d64 - mu) * iota
    e_xh = iota * (e_d + e_d.mean(0) + xh.abs() * (xh.abs() * e_d).mean(0))
    G, B = bn.weight.detach().double(), bn.bias.detach().double()
    ref = torch.relu(G * xh + B)
    zero = torch.zeros(256, dtype=torch.float64, device=DEV)
    e_mu, e_var, _ = BB.stats_bound(xb, zero, None)
    mu_b, var_b = BB.stats_ref(xb)
    iota_b, e_iota_b, hi_b = BB.invstd_interval(var_b, e_var, float(np.float32(bn.eps)))
    _, b_own = BB.apply_ref_bound(xb, mu_b, iota_b, e_mu, e_iota_b, hi_b, G, B)
    assert _excess(z.detach().reshape(N, 256), ref, G.abs() * e_xh * (1 + 1e-3) + b_own) <= 1.0


# ---- real steps: the pivot distance R and the bound at every train-mode BatchNorm -------------------------------------------------
def test_batchnorm_statistics_of_real_steps_meet_the_bound(monkeypatch):
    """R101 at 769^2, 2 + 2 images, eager: two states -- bench.py's calibrated workload and a random-init model at step 0 -- each
    one supervised-only step (Winograd on) and one semi-supervised step (Winograd off).  At every train-mode BatchNorm the pivot
    before the finalisation and the input are captured; mean, invstd, running statistics and y are held to the bound.  Per layer:
    M, C, route, the largest and 99th-percentile R, the largest error over the bound (written to U2PL_BN_STATS_OUT if set)."""
    import bench
    from test_gpu_split_bounds import _step_setup
    from u2pl_amd import nn as Kn
    monkeypatch.setenv("U2PL_GRAPHS", "0")
    saved = dict(Kn.CONV_ALGO)
    out_path = os.environ.get("U2PL_BN_STATS_OUT")
    S = 769
    layers, counts = {}, {}
    real = Kn.call
    try:
        for state in ("calibrated", "random_init"):
            tr, model, teacher = _step_setup(S, 7)
            gen = torch.Generator(device=DEV).manual_seed(7)
            batches = [bench.synth_batch(2, S, 19, DEV, gen) for _ in range(2)]
            if state == "calibrated":
                batches = bench.calibrate(model, teacher, batches, batches, 4.0)
            names = {m.running_mean.data_ptr(): tag + n for tag, mod in (("", model), ("teacher.", teacher))
                     for n, m in mod.named_modules() if isinstance(m, Kn.BatchNorm2d)}
            probe = BnProbe(real, backward=False, names=names)
            monkeypatch.setattr(Kn, "call", probe)
            for epoch, wino in ((0, saved["wino"] or 4), (1, 0)):
                Kn.CONV_ALGO.update(wino=wino)
                il, ll, iu = batches[epoch]
                m = tr.train_step(il, ll, iu, epoch=epoch)
                torch.cuda.synchronize()
                assert torch.isfinite(m).all(), m
            monkeypatch.setattr(Kn, "call", real)
            train = [r for r in probe.records if r.get("mode") == "train"]
            counts[state] = len(train)
            # every train-mode finalisation was followed by a checked apply; nothing train-mode went unattributed (the unknown
            # records left are the teacher's eval-mode applies with the one-launch invstd)
            finalized = probe.seen.get("u2pl_bn_finalize_f32", 0) + probe.seen.get("u2pl_bn_finish_finalize_f32", 0)
            assert len(train) == finalized, (state, len(train), finalized)
            assert not [u for u in probe.unknown if u.get("train")], (state, [u for u in probe.unknown if u.get("train")][:5])
            for r in train:
                key = (state, r["layer"])
                e = layers.setdefault(key, dict(state=state, layer=r["layer"], M=r["M"], C=r["C"], routes=set(), calls=0, R_max=0.0,
                                                R_p99=0.0, const_channels=0, max_excess=0.0, max_invstd_err_over_fp32_part=0.0))
                e["routes"].add(r["route"])
                e["calls"] += 1
                e["M"] = max(e["M"], r["M"])
                e["R_max"] = max(e["R_max"], r["R_max"])
                e["R_p99"] = max(e["R_p99"], r["R_p99"])
                e["const_channels"] = max(e["const_channels"], r["const_channels"])
                e["max_excess"] = max(e["max_excess"], max(r["excess"].values()))
                for k, v in r["excess"].items():
                    e.setdefault("excess", {})[k] = max(e.get("excess", {}).get(k, 0.0), v)
                e["max_invstd_err_over_fp32_part"] = max(e["max_invstd_err_over_fp32_part"], r["invstd_err_over_fp32_part"])
            assert not [r for r in train if r.get("mask_mismatch")], state
            del tr, model, teacher, probe
            torch.cuda.empty_cache()
    finally:
        monkeypatch.setattr(Kn, "call", real)
        Kn.CONV_ALGO.update(saved)
    rows = sorted(layers.values(), key=lambda e: (e["state"], e["layer"]))
    for e in rows:
        e["routes"] = sorted(e["routes"])
    fp32 = [e for e in rows if e["routes"] != ["small"]]
    print("train-mode BatchNorm calls per state:", counts)
    print("largest error / bound:", max(e["max_excess"] for e in rows),
          "largest R on the fp32 routes:", max((e["R_max"], e["layer"], e["state"]) for e in fp32),
          "on the float64 few-row route:", max((e["R_max"], e["layer"], e["state"]) for e in rows if e["routes"] == ["small"]))
    if out_path:
        with open(out_path, "w") as f:
            json.dump(dict(commit=os.environ.get("U2PL_COMMIT", ""), crop=S, images="2 + 2", calls_per_state=counts,
                           largest_excess=max(e["max_excess"] for e in rows),
                           largest_R_fp32_routes=max(e["R_max"] for e in fp32), layers=rows), f, indent=1)
    bad = [(e["state"], e["layer"], e["max_excess"]) for e in rows if not e["max_excess"] <= 1.0]
    assert not bad, bad
    # the pivot term of the fp32 routes stays below the variance term's 2^10 (R <= 32); above that the statistics would need
    # per-partial shifts.  The few-row route is float64: its R (up to ~1e5 on the pooled vectors) costs nothing there.
    far = [(e["state"], e["layer"], e["routes"], e["R_max"]) for e in fp32 if not e["R_max"] <= 32]
    assert not far, far
