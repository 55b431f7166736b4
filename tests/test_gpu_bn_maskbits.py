"""-m gpu: the ReLU mask of a BatchNorm with a residual as a bit plane (csrc/nn.hip: k_bn_apply_bits, BnBwdOp<3, ..>,
k_bn_bwd_apply_bits), through the C entry points, with the inputs of tests/test_gpu_bn_stream.py.

The forward's plane must be [stored y > 0] bit for bit (a zero Dropout2d scale gives a zero bit), y and max |y| must be the bytes
of the entry without bits, and no word outside [M][C / 32] may be written.  The two backward entries that read the plane must give
the BYTES of the entries that read y: sums, dx, dres, both maxima, the parameter gradients with and without accumulate, train
and eval.  No tolerance anywhere: the predicate is the same, only where it is read from differs.

Shapes: C / 4 = 8, 24 (does not divide 256), 64, 256 and 512 (two column slabs); rows that end inside a row group and inside the
unrolled rows; every float tensor with a pitch larger than C and the plane with a pitch larger than C / 32.  C = 48 has no bit
form: the entries return U2PL_EINVAL and nn._BNFn reads the mask from y."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_bn_stream import DEV, NHW, PAD, _call, _dev, _inputs, _out, _ws  # noqa: E402

pytestmark = pytest.mark.gpu
CS = (32, 96, 256, 1024, 2048)
SENTINEL = 0x5A5A5A5A            # what the plane's buffer holds before the launch
TAIL = 2                         # rows of the plane's buffer behind row M


def _plane(M, ldb):
    return torch.full((M + TAIL, ldb), SENTINEL, device=DEV, dtype=torch.int32)


def _packed(y, C):
    """[M, >= C] float32 on the device -> uint32 [M, C / 32]: bit c % 32 of word c / 32 = y[:, c] > 0"""
    b = (y[:, :C] > 0).cpu().numpy()
    return np.packbits(b.reshape(b.shape[0], C // 32, 32), axis=-1, bitorder="little").view("<u4").reshape(b.shape[0], C // 32)


def _check_plane(bits, M, C, y, what):
    got = bits.cpu().numpy().view(np.uint32)
    assert np.array_equal(got[:M, :C // 32], _packed(y, C)), what + ": bits"
    assert np.all(got[:M, C // 32:] == SENTINEL), what + ": padding words written"
    assert np.all(got[M:] == SENTINEL), what + ": words past row M written"


def _forward(d, C, ldx, ldr, ldy, ldb, relu, drop, vec):
    """y (pitch ldy), its amax object and the plane (pitch ldb) of the residual form, from u2pl_bn_apply_bits_f32"""
    M = d["M"]
    x, res = _dev(d["x"], ldx), _dev(d["res"], ldr)
    y, am, bits = _out(M, ldy), torch.zeros(2048, device=DEV), _plane(M, ldb)
    _call("u2pl_bn_apply_bits_f32", x, ldx, vec["mean"], vec["invstd"], vec["gamma"], vec["beta"], res, ldr, int(relu),
          vec["drop"] if drop else None, d["HW"], y, ldy, M, C, am, bits, ldb)
    return x, res, y, am, bits


@pytest.mark.parametrize("C", CS)
def test_forward_leaves_the_mask_of_the_stored_output(C):
    ldx, ldy, ldr, ldb = C + 32, C + 64, C + 4, C // 32 + 3
    for N, HW in NHW:
        d = _inputs(C, N, HW)
        M = d["M"]
        vec = {k: _dev(d[k]) for k in ("mean", "invstd", "gamma", "beta", "drop")}
        for relu, drop in ((1, False), (1, True), (0, False)):
            what = "C=%d N=%d HW=%d relu=%d drop=%d" % (C, N, HW, relu, drop)
            x, res, y, am, bits = _forward(d, C, ldx, ldr, ldy, ldb, relu, drop, vec)
            y0, am0 = _out(M, ldy), torch.zeros(2048, device=DEV)
            _call("u2pl_bn_apply_amax_f32", x, ldx, vec["mean"], vec["invstd"], vec["gamma"], vec["beta"], res, ldr, relu,
                  vec["drop"] if drop else None, HW, y0, ldy, M, C, am0)
            assert torch.equal(y.view(torch.int32), y0.view(torch.int32)), what + ": y"        # (padding included)
            assert torch.equal(am.view(torch.int32), am0.view(torch.int32)), what + ": max |y|"
            _check_plane(bits, M, C, y0, what)
            if drop:      # a zero scale: a zero bit, whatever the sign before it
                zero = torch.from_numpy(d["drop_rows"] == 0).to(DEV)
                assert bool(zero.any()) and not bool(((y0[:, :C] > 0) & zero).any()), what
            # without the maximum
            y1, bits1 = _out(M, ldy), _plane(M, ldb)
            _call("u2pl_bn_apply_bits_f32", x, ldx, vec["mean"], vec["invstd"], vec["gamma"], vec["beta"], res, ldr, relu,
                  vec["drop"] if drop else None, HW, y1, ldy, M, C, None, bits1, ldb)
            assert torch.equal(y1.view(torch.int32), y0.view(torch.int32)) and torch.equal(bits1, bits), what + " (no maximum)"
        # relu = 3 of the entries without bits (what nn._bn_apply launches): the plane packed behind y's last row, pitch C / 32
        for entry in ("u2pl_bn_apply_amax_f32", "u2pl_bn_apply_f32"):
            buf = torch.full((M * C + (M + TAIL) * (C // 32),), float(PAD), device=DEV)
            buf[M * C:].view(torch.int32).fill_(SENTINEL)
            am = torch.zeros(2048, device=DEV)
            xc, rc = _dev(d["x"]), _dev(d["res"])
            _call(entry, xc, C, vec["mean"], vec["invstd"], vec["gamma"], vec["beta"], rc, C, 3, None, HW, buf, C, M, C,
                  *((am,) if entry.endswith("amax_f32") else ()))
            yc = _out(M, C)
            _call("u2pl_bn_apply_f32", xc, C, vec["mean"], vec["invstd"], vec["gamma"], vec["beta"], rc, C, 1, None, HW, yc, C, M, C)
            assert torch.equal(buf[:M * C].view(M, C), yc), "%s relu=3 C=%d M=%d: y" % (entry, C, M)
            _check_plane(buf[M * C:].view(torch.int32).view(M + TAIL, C // 32), M, C, yc, "%s relu=3 C=%d M=%d" % (entry, C, M))


@pytest.mark.parametrize("C", CS)
def test_backward_sums_from_bits_are_the_bytes_of_the_sums_from_y(C):
    lddy, ldx, ldy, ldr, ldb = C + 4, C + 32, C + 64, C + 4, C // 32 + 3
    for N, HW in NHW:
        d = _inputs(C, N, HW)
        M = d["M"]
        vec = {k: _dev(d[k]) for k in ("mean", "invstd", "gamma", "beta", "drop")}
        dy, ws = _dev(d["dy"], lddy), _ws(M, C)
        for drop in (True, False):
            what = "C=%d N=%d HW=%d drop=%d" % (C, N, HW, drop)
            x, _, y, _, bits = _forward(d, C, ldx, ldr, ldy, ldb, 1, drop, vec)
            dr = vec["drop"] if drop else None
            want = torch.full((2 * C,), -1.0, device=DEV, dtype=torch.float64)
            _call("u2pl_bn_bwd_sums_f32", dy, lddy, x, ldx, y, ldy, vec["mean"], vec["invstd"], dr, HW, M, C, ws, want)
            got = torch.full((2 * C,), -2.0, device=DEV, dtype=torch.float64)
            _call("u2pl_bn_bwd_sums_bits_f32", dy, lddy, x, ldx, bits, ldb, vec["mean"], vec["invstd"], dr, HW, M, C, ws, got)
            assert torch.equal(got.view(torch.int64), want.view(torch.int64)), what
            assert bool((want[:C] != 0).any())       # (a mask of zeros would pass as well)


@pytest.mark.parametrize("C", CS)
def test_backward_apply_from_bits_gives_the_bytes_of_the_apply_from_y(C):
    lddy, ldx, ldy, ldr, lddx, lddr, ldb = C + 4, C + 32, C + 64, C + 4, C + 8, C + 12, C // 32 + 3
    for N, HW in NHW:
        d = _inputs(C, N, HW)
        M = d["M"]
        vec = {k: _dev(d[k]) for k in ("mean", "invstd", "gamma", "beta", "drop")}
        dy = _dev(d["dy"], lddy)
        psums = torch.from_numpy(d["psums"]).to(DEV)
        sums = torch.from_numpy(d["psums"][::-1].copy()).to(DEV)      # (any sums: both entries get the same)
        for drop in (True, False):
            x, _, y, _, bits = _forward(d, C, ldx, ldr, ldy, ldb, 1, drop, vec)
            dr = vec["drop"] if drop else None
            # the full cross with the Dropout2d scales; without them the 4 (dres, mode) forms
            combos = [(a, tr, pg, am) for a in (1, 0) for tr in (1, 0) for pg in (None, 0, 1) for am in (1, 0)
                      if drop or (pg is None and am == 1)]
            for want_dres, train, pg, maxima in combos:
                what = "C=%d N=%d HW=%d drop=%d dres=%d train=%d pg=%s maxima=%d" % (C, N, HW, drop, want_dres, train, pg, maxima)
                outs = []
                for form in ("y", "bits"):
                    dx, dres = _out(M, lddx), (_out(M, lddr) if want_dres else None)
                    ax, ar = (torch.zeros(2048, device=DEV), torch.zeros(2048, device=DEV)) if maxima else (None, None)
                    gs, bs = (_dev(d["sink0"][0].copy()), _dev(d["sink0"][1].copy())) if pg is not None else (None, None)
                    tail = (HW, sums if train else None, float(M), dx, lddx, dres, lddr, M, C, psums if pg is not None else None,
                            gs, bs, int(pg or 0), ax, ar)
                    if form == "y":
                        _call("u2pl_bn_bwd_apply_amax_f32", dy, lddy, x, ldx, y, ldy, vec["mean"], vec["invstd"], vec["gamma"], dr,
                              *tail, None)
                    else:
                        _call("u2pl_bn_bwd_apply_bits_f32", dy, lddy, x, ldx, bits, ldb, vec["mean"], vec["invstd"], vec["gamma"], dr,
                              *tail)
                    outs.append((dx, dres, ax, ar, gs, bs))
                for name, a, b in zip(("dx", "dres", "max |dx|", "max |dres|", "dgamma", "dbeta"), *outs):
                    assert (a is None) == (b is None)
                    if a is not None:      # (whole buffers: the padding behind each row as well)
                        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), what + ": " + name
                assert bool((outs[0][0][:, :C] != 0).any()), what


def test_48_channels_have_no_bit_form_and_the_layer_reads_y(monkeypatch):
    """C % 32 != 0: U2PL_EINVAL from the three entries (nothing launched); nn._BNFn then launches what it launched before the
    bit form.  C = 64 beside it: relu = 3 and the two entries from bits where a graph is recorded, the plain form under no_grad
    and under the switch -- and the same gradient bytes either way"""
    from u2pl_amd import nn as K
    from u2pl_amd._lib import HipError
    C, M = 48, 5
    f = torch.zeros(M, C, device=DEV)
    v = torch.ones(C, device=DEV)
    bits = torch.zeros(M, 2, device=DEV, dtype=torch.int32)
    d64 = torch.zeros(2 * C, device=DEV, dtype=torch.float64)
    for args in (("u2pl_bn_apply_bits_f32", f, C, v, v, v, v, f, C, 1, None, M, f.clone(), C, M, C, None, bits, 2),
                 ("u2pl_bn_bwd_sums_bits_f32", f, C, f, C, bits, 2, v, v, None, M, M, C, _ws(M, C), d64),
                 ("u2pl_bn_bwd_apply_bits_f32", f, C, f, C, bits, 2, v, v, v, None, M, d64, float(M), f.clone(), C, None, C, M, C,
                  None, None, None, 0, None, None)):
        with pytest.raises(HipError, match="1001"):
            _call(*args)

    seen = []
    real = K.call

    def spy(name, *a):
        if name.startswith("u2pl_bn_"):
            seen.append((name, a[8] if "apply" in name and "bwd" not in name else None))
        return real(name, *a)

    monkeypatch.setattr(K, "call", spy)
    saved = K.RELU_MASK_BITS
    g = torch.Generator(device=DEV).manual_seed(48)
    try:
        for C, bit_form in ((48, False), (64, True)):
            bn = K.BatchNorm2d(C).to(DEV)
            x0 = torch.randn(2, C, 5, 7, generator=g, device=DEV).contiguous(memory_format=torch.channels_last)
            r0 = torch.randn(2, C, 5, 7, generator=g, device=DEV).contiguous(memory_format=torch.channels_last)
            gy = torch.randn(2, C, 5, 7, generator=g, device=DEV).contiguous(memory_format=torch.channels_last)
            grads = {}
            stats = (bn.running_mean.clone(), bn.running_var.clone())
            for on in (True, False):
                K.RELU_MASK_BITS = on
                del seen[:]
                with torch.no_grad():      # (the running mean is the pivot of the statistics' sums: the same for both runs)
                    bn.running_mean.copy_(stats[0]), bn.running_var.copy_(stats[1])
                x, r = x0.clone().requires_grad_(True), r0.clone().requires_grad_(True)
                bn.weight.grad = bn.bias.grad = None
                y = bn(x, res=r, relu=True)
                y.backward(gy)
                torch.cuda.synchronize()
                names = [n for n, _ in seen]
                if on and bit_form:
                    assert [a for n, a in seen if a is not None] == [3], seen
                    assert "u2pl_bn_bwd_sums_bits_f32" in names and "u2pl_bn_bwd_apply_bits_f32" in names, seen
                else:
                    assert [a for n, a in seen if a is not None] == [1] and not [n for n in names if "bits" in n], seen
                    assert "u2pl_bn_bwd_sums_f32" in names, seen
                grads[on] = [t.detach().clone() for t in (y, x.grad, r.grad, bn.weight.grad, bn.bias.grad)]
            for a, b in zip(grads[True], grads[False]):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32))
            K.RELU_MASK_BITS = True
            del seen[:]
            with torch.no_grad():
                bn(x0, res=r0, relu=True)
            assert [a for n, a in seen if a is not None] == [1], seen        # no graph: no plane
    finally:
        K.RELU_MASK_BITS = saved
