"""The BatchNorm bound of tests/bn_bounds.py on the CPU: fp32 emulations of every statistics route in its kernel's summation
order (csrc/nn.hip stand-alone pass and float64 few-row pass, the igemm_ws.hip / conv.hip epilogues, the Winograd output
transform), followed by the finalisation, the apply and the backward, meet the bound at every pivot distance R (constant channels
included); and the bound rejects each mutant of that arithmetic.  (The GPU kernels are held to the same bound in
tests/test_gpu_bn_bounds.py.)"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn_bounds as BB  # noqa: E402

EPS_BN, MOM = 1e-5, 0.1
ROUTES = ("standalone", "igemm_ws", "igemm_ws+bias", "conv", "conv+bias", "wino4", "wino2", "small")


def _T(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64))


def _case(route, R, seed=0, sigma=1.0, M=None, C=None):
    """x [M, C] float32 with channel means / deviations of O(1) (times sigma), channel 0 constant; the pivot p = mu + R sigma
    (channel 0: p != its value); for the bias routes the accumulator and the bias, x = fl(acc + bias)"""
    rng = np.random.default_rng(seed)
    if M is None:      # not a multiple of any route's tile; the stand-alone pass: two column slabs, the second ragged (C4 = 65)
        M, C = {"standalone": (9000, 260), "small": (48, 16)}.get(route, (1037, 8))
    mu = rng.standard_normal(C) * 2
    sd = rng.uniform(0.5, 2.0, C) * sigma
    x = (mu + sd * rng.standard_normal((M, C))).astype(np.float32)
    x[:, 0] = np.float32(1.7)
    acc = bias = None
    if route.endswith("+bias"):
        bias = (rng.standard_normal(C) * 0.5).astype(np.float32)
        acc = (x - bias).astype(np.float32)
        x = (acc + bias).astype(np.float32)
    xd = x.astype(np.float64)
    sign = np.where(rng.random(C) < 0.5, -1.0, 1.0)
    p = (xd.mean(0) + R * xd.std(0) * sign).astype(np.float32)
    p[0] = np.float32(-0.3)
    return x, p, acc, bias, rng


def _stats(route, x, p, acc, bias, drop_last=False):
    """-> ((S1, S2) in double, L)"""
    M, C = x.shape
    if route == "small":
        return BB.emulate_small(x, p), None
    if route.startswith("wino"):
        mt = int(route[4])
        return BB.emulate_stats("wino", x, p, mt=mt, drop_last=drop_last), BB.L_wino(mt, C)
    base = route.split("+")[0]
    L = {"standalone": BB.L_standalone(M, C), "igemm_ws": BB.L_IGEMM_WS, "conv": BB.L_CONV}[base]
    return BB.emulate_stats(base, x, p, acc=acc, bias=bias, drop_last=drop_last), L


def run(route, R, relu=True, res=False, drop=False, sigma=1.0, stats_mut=None, fin_mut=None, apply_mut=None, bwd_mut=None,
        M=None, C=None, seed=0):
    """emulate one BatchNorm forward + backward of `route` and return each output's error over its bound, and the number of
    decided ReLU elements whose mask differs from float64"""
    x, p, acc, bias, rng = _case(route, R, seed, sigma, M, C)
    M, C = x.shape
    rv0 = rng.uniform(0.5, 2.0, C).astype(np.float32)
    gamma = (rng.random(C) + 0.5).astype(np.float32)
    beta = (rng.standard_normal(C) * 0.1).astype(np.float32)
    rs = rng.standard_normal((M, C)).astype(np.float32) if res else None
    dr = None
    if drop:       # a Dropout2d keep-mask of 4 images x C channels as a per-row scale
        keep = (rng.random((4, C)) > 0.3).astype(np.float32) / np.float32(0.7)
        dr = np.repeat(keep, -(-M // 4), 0)[:M]
    dy = rng.standard_normal((M, C)).astype(np.float32)
    (S1, S2), L = _stats(route, x, p, acc, bias, **(stats_mut or {}))
    mean, invstd, rm, rv = BB.emulate_finalize(S1, S2, M, p, EPS_BN, MOM, p, rv0, **(fin_mut or {}))
    y = BB.emulate_apply(x, mean, invstd, gamma, beta, rs, relu, dr, **(apply_mut or {}))
    dx, dres, S0k, S1k = BB.emulate_bwd(dy, x, y, mean, invstd, gamma, dr, relu, **(bwd_mut or {}))

    X, P = _T(x), _T(p)
    shift = BB.bias_shift_err(X, _T(bias), P) if bias is not None else None
    mu, var = BB.stats_ref(X)
    e_mu, e_var, e1 = BB.stats_bound(X, P, L, shift)
    iota, e_iota, hi = BB.invstd_interval(var, e_var, float(np.float32(EPS_BN)))
    rmr, brm, rvr, brv = BB.running_ref_bound(P, _T(rv0), mu, var, M, MOM, e1, e_var)
    G, B = _T(gamma), _T(beta)
    DR = _T(dr) if dr is not None else None
    pre, b = BB.apply_ref_bound(X, mu, iota, e_mu, e_iota, hi, G, B, _T(rs) if res else None)
    yr, by = BB.finish_y(pre, b, relu, DR)
    mask = _T(y > 0) if relu else 1.0          # the backward's mask: the kernel's own forward decision
    bw = BB.bwd_ref_bound(X, _T(dy), mask, DR, mu, iota, e_mu, e_iota, hi, G, BB.L_colreduce_chain(M, C))
    ex = dict(mean=BB.excess(mean, mu, e_mu), invstd=BB.excess(invstd, iota, e_iota), running_mean=BB.excess(rm, rmr, brm),
              running_var=BB.excess(rv, rvr, brv), y=BB.excess(y, yr, by), dx=BB.excess(dx, *bw["dx"]),
              dres=BB.excess(dres, *bw["dres"]), dbeta=BB.excess(S0k, *bw["S0"]), dgamma=BB.excess(S1k, *bw["S1"]))
    return ex, (BB.mask_mismatch(pre, b, _T(y), DR) if relu else 0)


@pytest.mark.parametrize("R", [0, 1, 10, 100, 1000])
@pytest.mark.parametrize("route", ROUTES)
def test_faithful_emulation_meets_the_bound_at_every_pivot_distance(route, R):
    """each route's own summation order, R = |mu - p| / sigma from 0 to 1000 (the variance bound carries (1 + R^2) sigma^2), a
    constant channel with p != its value, three forms of the apply (+res +ReLU, ReLU x drop, plain)"""
    for kw in (dict(relu=True, res=True), dict(relu=True, drop=True), dict(relu=False)):
        ex, mm = run(route, R, **kw)
        assert max(ex.values()) <= 1.0, (route, R, kw, ex)
        assert mm == 0, (route, R, kw, mm)


def test_route_chain_lengths_follow_the_kernels():
    """the L of each route as derived in bn_bounds.py, at the network's sizes (2 + 2 images at 769^2)"""
    assert BB.colreduce_geometry(592900, 64) == (512, 1159, [16])
    assert BB.L_standalone(592900, 64) == 1 + 19 + 3 + 2 + 15 + 1          # the stem: 385^2 x 4 rows
    assert BB.colreduce_geometry(841 * 2, 320)[2] == [4, 16]                # a ragged second column slab
    assert BB.colreduce_geometry(961 * 3, 36)[2] == [28]                    # C/4 = 9: 28 row groups, 4 idle threads
    assert BB.L_IGEMM_WS == 21 and BB.L_CONV == 37
    assert BB.L_wino(4, 256) == 20 and BB.L_wino(2, 256) == 8


def test_float64_few_row_route_is_held_to_double_precision():
    """M <= 64 (the ASPP image-pool rows, which differ by ~1 %: R ~ 100 with the pivot at 0): the bound of the float64 two-pass
    kernel is below 2^-20 of the fp32 routes' at the same data, and the fp32 stand-alone order on those rows misses it"""
    rng = np.random.default_rng(3)
    C = 16
    base = rng.uniform(0.5, 2.0, C)
    x = (base * (1 + 0.01 * rng.standard_normal((64, C)))).astype(np.float32)
    p = np.zeros(C, dtype=np.float32)
    X, P = _T(x), _T(p)
    mu, var = BB.stats_ref(X)
    assert float(((mu - P).abs() / var.sqrt()).min()) > 30
    _, e_small, _ = BB.stats_bound(X, P, None)
    _, e_f32, _ = BB.stats_bound(X, P, BB.L_standalone(64, C))
    assert float((e_small / e_f32).max()) < 2.0 ** -20
    iota, e_iota, _ = BB.invstd_interval(var, e_small, float(np.float32(EPS_BN)))
    S1, S2 = BB.emulate_small(x, p)
    _, invstd, _, _ = BB.emulate_finalize(S1, S2, 64, p, EPS_BN, MOM, p, np.ones(C, np.float32))
    assert BB.excess(invstd, iota, e_iota) <= 1.0
    S1, S2 = BB.emulate_stats("standalone", x, p)
    _, invstd32, _, _ = BB.emulate_finalize(S1, S2, 64, p, EPS_BN, MOM, p, np.ones(C, np.float32))
    assert BB.excess(invstd32, iota, e_iota) > 1.0


# mutant -> (route, R, run() keyword arguments, the outputs that must catch it).  Each is visible on its data by a wide margin:
# a small variance for eps, R = 10 where the pivot or the momentum enters, M not a multiple of the tile for the dropped block,
# R = 100 on few rows for the fp32 finish.
MUTANTS = {
    "biased running_var": ("standalone", 0, dict(fin_mut=dict(biased_rv=True), M=300, C=8), ("running_var",)),
    "eps outside the square root": ("igemm_ws", 0, dict(fin_mut=dict(eps_outside=True), sigma=0.01), ("invstd", "y")),
    "count = M - 1": ("standalone", 10, dict(fin_mut=dict(count=1036), M=1037, C=8), ("mean",)),
    "last partial block dropped": ("igemm_ws", 0, dict(stats_mut=dict(drop_last=True)), ("mean", "invstd")),
    "last partial block dropped (Winograd)": ("wino4", 0, dict(stats_mut=dict(drop_last=True), M=5000, C=64), ("mean",)),
    "last partial block dropped (stand-alone)": ("standalone", 0, dict(stats_mut=dict(drop_last=True)), ("mean",)),
    "pivot read after the running-mean update": ("conv", 10, dict(fin_mut=dict(pivot_after=True)), ("mean", "y")),
    "m and 1 - m swapped": ("wino4", 10, dict(fin_mut=dict(swap_m=True)), ("running_mean", "running_var")),
    "mask taken as y >= 0": ("standalone", 0, dict(bwd_mut=dict(mask_ge=True), relu=True), ("dx", "dgamma")),
    "drop applied twice": ("igemm_ws", 0, dict(apply_mut=dict(drop_twice=True), relu=True, drop=True), ("y",)),
    "S0 and S1 swapped in the backward apply": ("standalone", 1, dict(bwd_mut=dict(swap_sums=True), relu=False), ("dx",)),
    "dres written without the mask": ("conv", 0, dict(bwd_mut=dict(dres_unmasked=True), relu=True, res=True), ("dres",)),
    "finish in fp32 instead of double": ("small", 100, dict(fin_mut=dict(fp32=True), relu=True), ("invstd",)),
}


@pytest.mark.parametrize("name", list(MUTANTS))
def test_bound_rejects_the_mutant(name):
    route, R, kw, catchers = MUTANTS[name]
    faithful = {k: v for k, v in kw.items() if not k.endswith("_mut")}
    ex, mm = run(route, R, **faithful)
    assert max(ex.values()) <= 1.0 and mm == 0, (name, "faithful", ex)
    ex, _ = run(route, R, **kw)
    assert max(ex[c] for c in catchers) > 1.0, (name, ex)
