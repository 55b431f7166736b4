"""-m gpu: the BatchNorm passes of csrc/nn.hip (k_bn_apply, k_bn_bwd_apply, k_colreduce_partial) held BIT FOR BIT to the fp32
emulations of tests/bn_bounds.py (emulate_apply, emulate_bwd, emu_colreduce), through the C entry points, at the smallest shapes
where the kernels' indexing can go wrong: C / 4 = 4, 12 (does not divide 256), 16, 64, 256 and 512 (two column slabs); rows that
end inside a row group and inside the unrolled rows; image boundaries (Dropout2d scales) inside a row group; every tensor with a
pitch larger than C.  The padding behind every output row must stay untouched, and the fused maxima must equal max |output|.

One large case: a tensor of more than 2^31 bytes (the row base is a 64-bit product), compared with torch eager on the device."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn_bounds as BB  # noqa: E402
from test_gpu_bn_bounds import VARIANTS  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
CS = (16, 48, 64, 256, 1024, 2048)
NHW = ((1, 1), (3, 7), (2, 129), (1, 1031))
PAD = np.float32(-7.5)           # what the padding of an output buffer holds before the launch
f32 = BB._f


def _call(*a):
    from u2pl_amd._lib import call
    call(*a)


def _ws(M, C):
    from u2pl_amd._lib import query
    return torch.empty(max(1, query("u2pl_colreduce_workspace_bytes", M, 1, C)), device=DEV, dtype=torch.uint8)


@functools.lru_cache(maxsize=None)
def _inputs(C, N, HW):
    """seeded CPU inputs of one layer: activations [M, C], per-channel vectors, Dropout2d scales [N, C]"""
    g = np.random.default_rng(1000 * C + 10 * HW + N)
    M = N * HW
    d = dict(M=M, HW=HW)
    for k in ("x", "res", "dy", "yprev"):
        d[k] = f32(g.standard_normal((M, C)))
    d["x"] = f32(d["x"] * 1.5 + 0.25)
    d["mean"] = f32(g.standard_normal(C) * 0.3)
    d["invstd"] = f32(g.uniform(0.5, 1.5, C))
    d["gamma"] = f32(g.standard_normal(C))
    d["beta"] = f32(g.standard_normal(C) * 0.5)
    d["drop"] = f32(np.where(g.uniform(size=(N, C)) < 0.3, 0.0, 1.0 / 0.9))
    d["drop_rows"] = np.repeat(d["drop"], HW, axis=0)
    d["psums"] = g.standard_normal(2 * C) * 100.0
    d["sink0"] = f32(g.standard_normal((2, C)))
    return d


def _dev(a, ld=None):
    """[M, C] float32 -> a device buffer of pitch ld (padding PAD)"""
    a = np.asarray(a)
    if ld is None:
        return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    buf = np.full((a.shape[0], ld), PAD, dtype=np.float32)
    buf[:, :a.shape[1]] = a
    return torch.from_numpy(buf).to(DEV)


def _out(M, ld):
    return torch.full((M, ld), float(PAD), device=DEV)


def _check_rows(buf, C, ref, what):
    got = buf.cpu().numpy()
    assert np.array_equal(got[:, :C], ref), what
    assert np.all(got[:, C:] == PAD), what + ": padding written"


def _check_amax(obj, ref, what):
    """the amax object (64 shards of uint32 bit patterns) against max |ref|"""
    got = int(obj.view(torch.int32).max())
    want = int(np.abs(ref).max().astype(np.float32).view(np.uint32)) if ref.size else 0
    assert got == want, what


@pytest.mark.parametrize("C", CS)
def test_apply_is_bit_equal_to_the_emulation(C):
    ldx, ldy, ldr = C + 32, C + 64, C + 4
    for N, HW in NHW:
        d = _inputs(C, N, HW)
        M = d["M"]
        x, res = _dev(d["x"], ldx), _dev(d["res"], ldr)
        vec = {k: _dev(d[k]) for k in ("mean", "invstd", "gamma", "beta", "drop")}
        for name, (has_res, relu, drop) in VARIANTS.items():
            what = "C=%d N=%d HW=%d %s" % (C, N, HW, name)
            ref = BB.emulate_apply(d["x"], d["mean"], d["invstd"], d["gamma"], d["beta"], d["res"] if has_res else None, relu,
                                   d["drop_rows"] if drop else None)
            y, am = _out(M, ldy), torch.zeros(2048, device=DEV)
            _call("u2pl_bn_apply_amax_f32", x, ldx, vec["mean"], vec["invstd"], vec["gamma"], vec["beta"], res if has_res else None,
                  ldr, int(relu), vec["drop"] if drop else None, HW, y, ldy, M, C, am)
            _check_rows(y, C, ref, what)
            _check_amax(am, ref, what + ": amax")
            y2 = _out(M, ldy)
            _call("u2pl_bn_apply_f32", x, ldx, vec["mean"], vec["invstd"], vec["gamma"], vec["beta"], res if has_res else None,
                  ldr, int(relu), vec["drop"] if drop else None, HW, y2, ldy, M, C)
            _check_rows(y2, C, ref, what + " (no maxima)")


@functools.lru_cache(maxsize=None)
def _bwd_ref(C, N, HW, mask, drop):
    """(y the mask is read from or None, dx train, dx eval, dres, double sums [2C]) of one backward"""
    d = _inputs(C, N, HW)
    if mask == "y":       # (any forward output: here the residual form's)
        y = BB.emulate_apply(d["x"], d["mean"], d["invstd"], d["gamma"], d["beta"], d["res"], True)
    elif mask == "x":     # y = relu(BN(x)), which the kernels recompute from x
        y = BB.emulate_apply(d["x"], d["mean"], d["invstd"], d["gamma"], d["beta"], None, True)
    else:
        y = d["yprev"]
    dx, dres, S0, S1 = BB.emulate_bwd(d["dy"], d["x"], y, d["mean"], d["invstd"], d["gamma"], d["drop_rows"] if drop else None,
                                      relu=mask != "none")
    dx_eval = f32(f32(d["gamma"] * d["invstd"]) * dres)
    return y, dx, dx_eval, dres, np.concatenate([S0, S1])


@pytest.mark.parametrize("C", CS)
def test_backward_sums_are_bit_equal_to_the_emulation(C):
    lddy, ldx, ldy = C + 4, C + 32, C + 64
    for N, HW in NHW:
        d = _inputs(C, N, HW)
        M = d["M"]
        dy, x = _dev(d["dy"], lddy), _dev(d["x"], ldx)
        vec = {k: _dev(d[k]) for k in ("mean", "invstd", "gamma", "beta", "drop")}
        ws = _ws(M, C)
        for mask in ("y", "x", "none"):
            for drop in (True, False):
                what = "C=%d N=%d HW=%d mask=%s drop=%d" % (C, N, HW, mask, drop)
                yref, _, _, _, S = _bwd_ref(C, N, HW, mask, drop)
                out = torch.full((2 * C,), -1.0, device=DEV, dtype=torch.float64)
                dr = vec["drop"] if drop else None
                if mask == "x":
                    _call("u2pl_bn_bwd_sums_mx_f32", dy, lddy, x, ldx, vec["mean"], vec["invstd"], vec["gamma"], vec["beta"], dr, HW,
                          M, C, ws, out)
                else:
                    _call("u2pl_bn_bwd_sums_f32", dy, lddy, x, ldx, _dev(yref, ldy) if mask == "y" else None, ldy, vec["mean"],
                          vec["invstd"], dr, HW, M, C, ws, out)
                assert np.array_equal(out.cpu().numpy(), S), what
        # the other two users of the column reduction: BatchNorm statistics (more than 64 rows) and plain column sums
        out = torch.full((2 * C,), -1.0, device=DEV, dtype=torch.float64)
        _call("u2pl_colsum_f32", x, ldx, M, 1, C, ws, out)
        assert np.array_equal(out.cpu().numpy(), np.concatenate([BB.emu_colreduce(d["x"]), np.zeros(C)])), "colsum C=%d M=%d" % (C, M)
        if M > BB.SMALL_M:
            _call("u2pl_bn_stats_f32", x, ldx, M, C, vec["mean"], ws, out)
            assert np.array_equal(out.cpu().numpy(), np.concatenate(BB.emulate_stats("standalone", d["x"], d["mean"]))), \
                "stats C=%d M=%d" % (C, M)


@pytest.mark.parametrize("C", CS)
def test_backward_apply_is_bit_equal_to_the_emulation(C):
    lddy, ldx, ldy, lddx, lddr = C + 4, C + 32, C + 64, C + 8, C + 12
    for N, HW in NHW:
        d = _inputs(C, N, HW)
        M = d["M"]
        dy, x = _dev(d["dy"], lddy), _dev(d["x"], ldx)
        vec = {k: _dev(d[k]) for k in ("mean", "invstd", "gamma", "beta", "drop")}
        psums = torch.from_numpy(d["psums"]).to(DEV)
        pg_ref = {acc: (f32((d["sink0"][0] if acc else np.float32(0)) + f32(d["psums"][C:])),
                        f32((d["sink0"][1] if acc else np.float32(0)) + f32(d["psums"][:C]))) for acc in (0, 1)}
        for mask in ("y", "x", "none"):
            for drop in (True, False):
                yref, dx_train, dx_eval, g, S = _bwd_ref(C, N, HW, mask, drop)
                y = _dev(yref, ldy) if mask == "y" else None
                sums = torch.from_numpy(S).to(DEV)
                # the full cross with the Dropout2d scales; without them the 4 (dres, mode) forms
                combos = [(dr, tr, pg, am) for dr in (1, 0) for tr in (1, 0) for pg in (None, 0, 1) for am in (1, 0)
                          if drop or (pg is None and am == 1)]
                for want_dres, train, pg, maxima in combos:
                    what = "C=%d N=%d HW=%d mask=%s drop=%d dres=%d train=%d pg=%s maxima=%d" % (C, N, HW, mask, drop, want_dres,
                                                                                               train, pg, maxima)
                    dx, dres = _out(M, lddx), (_out(M, lddr) if want_dres else None)
                    ax, ar = (torch.zeros(2048, device=DEV), torch.zeros(2048, device=DEV)) if maxima else (None, None)
                    gs, bs = (_dev(d["sink0"][0].copy()), _dev(d["sink0"][1].copy())) if pg is not None else (None, None)
                    _call("u2pl_bn_bwd_apply_amax_f32", dy, lddy, x, ldx, y, ldy, vec["mean"], vec["invstd"], vec["gamma"],
                          vec["drop"] if drop else None, HW, sums if train else None, float(M), dx, lddx, dres, lddr, M, C,
                          psums if pg is not None else None, gs, bs, int(pg or 0), ax, ar, vec["beta"] if mask == "x" else None)
                    ref = dx_train if train else dx_eval
                    _check_rows(dx, C, ref, what + ": dx")
                    if want_dres:
                        _check_rows(dres, C, g, what + ": dres")
                    if maxima:
                        _check_amax(ax, ref, what + ": dx amax")
                        _check_amax(ar, g, what + ": dres amax")
                    if pg is not None:
                        assert np.array_equal(gs.cpu().numpy(), pg_ref[pg][0]), what + ": dgamma"
                        assert np.array_equal(bs.cpu().numpy(), pg_ref[pg][1]), what + ": dbeta"


def test_apply_on_a_tensor_of_more_than_2_31_bytes():
    """C = 256, M * ld * 4 > 2^31: the last 4096 rows against the same expression in torch eager fp32 (separate element-wise
    kernels: no contraction)"""
    C, M, T = 256, (1 << 21) + 5000, 4096
    assert M * C * 4 > 2 ** 31
    g = torch.Generator(device=DEV).manual_seed(5)
    x = torch.randn(M, C, device=DEV, generator=g)
    mean, gamma, beta = (torch.randn(C, device=DEV, generator=g) for _ in range(3))
    invstd = torch.rand(C, device=DEV, generator=g) + 0.5
    drop = (torch.rand(2, C, device=DEV, generator=g) > 0.3).float() / 0.9
    rpi = M // 2 + 1                                    # the second image starts inside the tensor's second half
    y = torch.empty(M, C, device=DEV)
    am = torch.zeros(2048, device=DEV)
    _call("u2pl_bn_apply_amax_f32", x, C, mean, invstd, gamma, beta, None, 0, 1, drop, rpi, y, C, M, C, am)
    ref = ((x[M - T:] - mean) * invstd * gamma + beta).clamp_min(0.0) * drop[1]
    assert torch.equal(y[M - T:], ref)
    head = ((x[:T] - mean) * invstd * gamma + beta).clamp_min(0.0) * drop[0]
    assert torch.equal(y[:T], head)
    assert int(am.view(torch.int32).max()) == int(y.abs().max().view(torch.int32))
